"""Mask Scoring R-CNN's MaskIoU head (Huang et al., CVPR 2019): regresses, per class, the IoU between the mask the FCN
head predicts for a roi and its ground truth; at test time the mask score is the box score times that IoU.

Plugin slot: models/mask_heads (/root/reference/README.md:30) with core/mask (README.md:18). Input [R,14,14,320]: the
mask RoI features (256), the 2x2 max-pooled 28x28 mask probability of the roi's class (1), zeros up to a multiple of 64
(core.mask.maskiou_input) -> 3 x (conv3x3 256 + ReLU) -> conv3x3 stride 2 + ReLU -> [R,7,7,256] -> FC 1024 + ReLU ->
FC 1024 + ReLU -> FC num_classes-1 (padded to 128 columns); bias everywhere, no GroupNorm. L2 loss on the class column of
the rows with a positive target (core.mask.maskiou_target / maskiou_loss). The mask channel is a constant in the
backward pass: the head's gradient reaches the mask RoI features only.
"""
import os

import torch

from ...core import mask as M_
from ...ops import dense
from ..utils.layers import ConvLayer, cached_buf


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
        self.fc_out = ConvLayer("maskiou.fc_out", fc_dim, self.ld, 1, init_std=0.001, cout_real=num_classes - 1, **kw)
        self.fc2 = ConvLayer("maskiou.fc2", fc_dim, fc_dim, 1, **kw)
        self.fc1 = ConvLayer("maskiou.fc1", self.in_features, fc_dim, 1, **kw)
        self.fc1.fc_in_hwc = (h, h, channels)       # checkpoint layout, as bbox.fc1
        self.fc2.fc_in_hwc = ()
        self.fc_out.fc_in_hwc = ()
        self.convs = [None] * num_convs
        for i in reversed(range(num_convs)):
            last = i == num_convs - 1
            self.convs[i] = ConvLayer("maskiou.conv%d" % i, self.cin if i == 0 else channels, channels, 3,
                                      stride=2 if last else 1, **kw)
        # the alignment channels behind the mask channel see zero activations: zero filter entries stay zero
        self.convs[0]._w0[..., channels + 1:] = 0
        self.fc1_ksplit = int(os.environ.get("MXDET_TUNE_FC1_KSPLIT", "4"))
        self.bufs = {}

    def layers(self):
        return [self.fc_out, self.fc2, self.fc1] + list(reversed(self.convs))

    def norm_layers(self):
        return []

    def _buf(self, key, shape, dtype=torch.bfloat16, zero=False):
        return cached_buf(self.bufs, key, shape, dtype, self.device, zero)

    def plan(self, N, g_max=None):
        R = N * self.Rimg
        h = self.S // 2
        shp = (R, h, h, self.cin)
        for c in self.convs:
            c.plan(shp)
            shp = c.out_shape(shp)
        self.fc1.plan((R, 1, 1, self.in_features))
        self.fc2.plan((R, 1, 1, self.fc_dim))
        self.fc_out.plan((R, 1, 1, self.fc_dim))
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
        self.acts = [x]
        for i, c in enumerate(self.convs):
            x = c.forward(x, relu=True, out=self._buf("a%d" % i, c.out_shape(x.shape)))
            self.acts.append(x)
        self.x = x.view(R, 1, 1, -1)
        # fc1 under the box head's split-K rule (BBoxHead.forward)
        ks = self.fc1_ksplit if (R * self.fc_dim) % (64 * 64 * 8) == 0 and R % 64 == 0 else 1
        if ks > 1:
            ws = self._buf("fc1_ws", (4 * ks * R * self.fc_dim,), dtype=torch.uint8)
            self.h1 = dense.conv2d_forward_splitk(self.x, self.fc1.w_bf16, self.fc1.bias_f32, None, True, ks,
                                                  self._buf("h1", (R, 1, 1, self.fc_dim)), ws)
        else:
            self.h1 = self.fc1.forward(self.x, relu=True, out=self._buf("h1", (R, 1, 1, self.fc_dim)))
        self.h2 = self.fc2.forward(self.h1, relu=True, out=self._buf("h2", (R, 1, 1, self.fc_dim)))
        self.o = self.fc_out.forward(self.h2, out=self._buf("o", (R, 1, 1, self.ld)))
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
        self.fc_out.backward_weight(self.h2, self.go)
        d_h2 = self.fc_out.backward_data(self.go, self.h2.shape, relu_mask=self.h2, out=self._buf("dh2", self.h2.shape))
        self.fc2.backward_weight(self.h1, d_h2)
        d_h1 = self.fc2.backward_data(d_h2, self.h1.shape, relu_mask=self.h1, out=self._buf("dh1", self.h1.shape))
        self.fc1.backward_weight(self.x, d_h1)
        last = self.acts[-1]
        g = self.fc1.backward_data(d_h1, self.x.shape, relu_mask=last.view(self.x.shape),
                                   out=self._buf("dx", self.x.shape)).view(last.shape)
        for i in reversed(range(len(self.convs))):
            xin = self.acts[i]
            self.convs[i].backward_weight(xin, g)
            g = self.convs[i].backward_data(g, xin.shape, relu_mask=xin if i > 0 else None,
                                            out=self._buf("g%d" % i, xin.shape))
        return g
