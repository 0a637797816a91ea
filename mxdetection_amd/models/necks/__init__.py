"""models/necks (/root/reference/README.md:31)."""
from .bfp import BFP, check_neck  # noqa: F401
from .fpn import FPN, check_upsample  # noqa: F401
