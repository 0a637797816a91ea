"""Mask Scoring R-CNN's MaskIoU head (Huang et al., CVPR 2019): regresses, per class, the IoU between the mask the FCN
head predicts for a roi and its ground truth; at test time the mask score is the box score times that IoU.

Plugin slot: models/mask_heads (/root/reference/README.md:30) with core/mask (README.md:18). Input [R,14,14,320]: the
mask RoI features (256), the 2x2 max-pooled 28x28 mask probability of the roi's class (1), zeros up to a multiple of 64
(core.mask.maskiou_input) -> 3 x (conv3x3 256 + ReLU) -> conv3x3 stride 2 + ReLU -> [R,7,7,256] -> FC 1024 + ReLU ->
FC 1024 + ReLU -> FC num_classes-1 (padded to 128 columns); bias everywhere, no GroupNorm. L2 loss on the class column of
the rows with a positive target (core.mask.maskiou_target / maskiou_loss). The mask channel is a constant in the
backward pass: the head's gradient reaches the mask RoI features only.
"""
import torch

from ...core import mask as M_
from ..utils.layers import LayerChain, buf_cache


class MaskIoUHead:
    def __init__(self, channels, arena, ws, device, gen, num_classes=81, num_convs=4, size=28, rois_per_image=128,
                 fc_dim=1024, weight=1.0):
        kw = dict(arena=arena, ws=ws, device=device, gen=gen)
        self.nc, self.S, self.Rimg, self.device, self.C = num_classes, size, rois_per_image, device, channels
        self.cin = M_.MASKIOU_CIN
        assert channels < self.cin and self.cin % 64 == 0
        self.weight, self.fc_dim = float(weight), fc_dim
        self.ld = (num_classes - 1 + 63) // 64 * 64
        h = size // 4
        self.in_features = h * h * channels
        # registration = backward completion order
        # the output layer starts as small as mask.logits does: the loss is an unbounded L2, and a prediction far from
        # [0, 1] at the start sends a large gradient through the shared RoI features into the FPN (with std 0.01 on a
        # randomly initialised backbone the whole step diverged within three iterations at lr 0.002)
        fcs = [dict(name="maskiou.fc1", cin=self.in_features, cout=fc_dim, k=1, split=True),    # the box heads' split rule
               dict(name="maskiou.fc2", cin=fc_dim, cout=fc_dim, k=1),
               dict(name="maskiou.fc_out", cin=fc_dim, cout=self.ld, k=1, init_std=0.001, cout_real=num_classes - 1,
                    relu=False)]
        self.fcs = LayerChain(fcs, **kw)
        self.fc1, self.fc2, self.fc_out = self.fcs.convs
        self.fc1.fc_in_hwc = (h, h, channels)       # checkpoint layout, as bbox.fc1
        self.fc2.fc_in_hwc = ()
        self.fc_out.fc_in_hwc = ()
        self.tower = LayerChain([dict(name="maskiou.conv%d" % i, cin=channels if i else self.cin, cout=channels, k=3,
                                      stride=2 if i == num_convs - 1 else 1) for i in range(num_convs)], **kw)
        self.convs = self.tower.convs
        # the alignment channels behind the mask channel see zero activations: zero filter entries stay zero
        self.convs[0]._w0[..., channels + 1:] = 0
        self.bufs, self._buf = buf_cache(device)

    def layers(self):
        return self.fcs.layers() + self.tower.layers()

    def norm_layers(self):
        return []

    def plan(self, N, g_max=None):
        R = N * self.Rimg
        h = self.S // 2
        self.tower.plan((R, h, h, self.cin))
        self.fcs.plan((R, 1, 1, self.in_features))
        self.loss = torch.zeros((1,), dtype=torch.float32, device=self.device)
        if g_max is not None:      # the masks hold at most as many instances per image as the boxes
            self._target_ws(N, g_max)

    def _target_ws(self, N, G):
        """Workspace of maskiou_target for N x G instances: grown, never freed (a captured step holds it by address)."""
        need = M_.maskiou_target_workspace_bytes(N, G)
        ws = self.bufs.get("tgt_ws")
        if ws is None or ws.numel() < need:
            self.bufs.setdefault("tgt_ws_retired", []).append(ws)
            ws = self.bufs["tgt_ws"] = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return ws

    def forward(self, mpooled, mask_logits, cls):
        """mpooled bf16 [R,14,14,C]; mask_logits bf16 [R,28,28,Cpad]; cls [R] i32 (class 1.., <= 0: no mask channel).
        Returns the per-class IoU predictions bf16 [R,1,1,ld]."""
        R, h = mpooled.shape[0], mpooled.shape[1]
        x = M_.maskiou_input(mpooled, mask_logits, cls, out=self._buf("x", (R, h, h, self.cin)))
        self.cls = cls
        self.x = self.tower.forward(x, self._buf).view(R, 1, 1, -1)
        self.o = self.fcs.forward(self.x, self._buf)
        self.acts, self.h1 = self.tower.acts, self.fcs.acts[1]
        return self.o

    def targets(self, mask_head, gt_boxes, gt_masks):
        """The regression targets f32 [R] of the mask head's current rois, logits and mask targets."""
        R = mask_head.rois.shape[0]
        N, G = gt_masks.shape[:2]
        ws = self._target_ws(N, G)
        self.t =M_.maskiou_target(mask_head.rois, mask_head.matched, mask_head.cls, gt_boxes, gt_masks, mask_head.o,
                                   mask_head.tg, out=self._buf("t", (R,), torch.float32), workspace=ws)
        return self.t

    def loss_and_grad(self, loss_scale=1.0):
        R = self.o.shape[0]
        self.go = self._buf("go", self.o.shape)
        M_.maskiou_loss(self.o.view(R, self.ld), self.cls, self.t, self.loss, self.go.view(R, self.ld), loss_scale,
                        self.weight)
        return self.loss

    def backward(self):
        """Returns d(loss)/d(head input) bf16 [R,14,14,320]; channels [0,C) belong to the mask RoI features
        (core.mask.maskiou_input_bwd), the rest (mask channel, alignment padding) is dropped by the caller."""
        g = self.fcs.backward(self.go, self._buf, first_mask=self.tower.out_mask.view(self.x.shape))
        return self.tower.backward(g.view(self.acts[-1].shape), self._buf)
