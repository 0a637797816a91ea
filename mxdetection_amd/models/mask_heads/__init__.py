"""models/mask_heads (/root/reference/README.md:30)."""
from .fcn_mask_head import FCNMaskHead, select_rois  # noqa: F401
from .keypoint_head import KeypointHead  # noqa: F401
from .mask_iou_head import MaskIoUHead  # noqa: F401
