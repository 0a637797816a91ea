"""Keypoint R-CNN's keypoint head (He et al., Mask R-CNN, ICCV 2017, section 5): RoIAlign 14x14 on the foreground rois ->
8 x (conv3x3 512 + ReLU) -> deconv 2x2/2 -> per-keypoint 28x28 logits; at the loss and at test time the logits are seen
through a fixed x2 bilinear upsample (56x56), a one-hot target per keypoint and a softmax over the whole map.

Plugin slot: models/mask_heads (/root/reference/README.md:30) with core/mask (README.md:18). The deconvolution runs as a
1x1 convolution 512 -> 4*Kpad on the MFMA kernel followed by a pixel shuffle, as the mask head's does, without a ReLU; the K
keypoint channels are padded to Kpad (a multiple of 16: 32 for K = 17) so that dgrad's reduction dim 4*Kpad is a multiple of
64. The 2x2 kernel deviates from Detectron's 4x4 deconvolution. The 56x56 map exists only inside the loss
and decode kernels (core.mask.keypoint_loss / keypoint_decode).
"""
import torch

from ...core import mask as M_
from ...ops import dense
from ..utils.layers import ConvLayer, LayerChain, buf_cache
from .fcn_mask_head import select_rois


class KeypointHead:
    select_rois = select_rois      # the mask head's rule: background / padding rows are marked as not trained

    def __init__(self, channels, arena, ws, device, gen, num_keypoints=17, num_convs=8, conv_channels=512, size=28,
                 rois_per_image=128, weight=1.0):
        kw = dict(arena=arena, ws=ws, device=device, gen=gen)
        self.K, self.S, self.Rimg, self.device = int(num_keypoints), size, rois_per_image, device
        self.C, self.Cc = channels, conv_channels
        self.weight = float(weight)
        self.kpad = (self.K + 15) // 16 * 16
        # registration = backward completion order
        self.deconv = ConvLayer("kpt.deconv", conv_channels, 4 * self.kpad, 1, init_std=0.001, **kw)   # 2x2/2 deconv
        # output channel (dy*2+dx)*Kpad + c: the alignment channels c >= K start at zero and, with zero gradients from the
        # loss kernel, stay there
        self.deconv._w0.view(4, self.kpad, -1)[:, self.K:] = 0
        self.tower = LayerChain([dict(name="kpt.conv%d" % i, cin=conv_channels if i else channels, cout=conv_channels, k=3)
                                 for i in range(num_convs)], **kw)
        self.convs = self.tower.convs
        self.bufs, self._buf = buf_cache(device)

    def layers(self):
        return [self.deconv] + self.tower.layers()

    def norm_layers(self):
        return []

    def plan(self, N):
        R = N * self.Rimg
        h = self.S // 2
        self.deconv.plan(self.tower.plan((R, h, h, self.C)))
        self.loss = torch.zeros((1,), dtype=torch.float32, device=self.device)
        self.loss_ws = M_.keypoint_loss_workspace(R, self.device)

    def targets(self, gt_keypoints):
        """gt_keypoints f32 [N,G,K,3] -> the heatmap targets int32 [R,K] of the selected rois."""
        assert gt_keypoints.shape[2] == self.K, "gt_keypoints carries %d keypoints, the head %d" % (gt_keypoints.shape[2], self.K)
        R = self.rois.shape[0]
        self.tg = M_.keypoint_target(self.rois, self.matched, self.roi_labels, gt_keypoints, self.S,
                                     out=self._buf("tg", (R, self.K), torch.int32))
        return self.tg

    def forward(self, pooled):
        """pooled bf16 [R,14,14,C] -> logits bf16 [R,28,28,Kpad]"""
        x = self.tower.forward(pooled, self._buf)
        self.acts = self.tower.acts
        R, h, w, _ = x.shape
        self.d4 = self.deconv.forward(x, out=self._buf("d4", (R, h, w, 4 * self.kpad)))
        self.o = dense.pixel_shuffle2(self.d4, self._buf("o", (R, 2 * h, 2 * w, self.kpad)))
        return self.o

    def loss_and_grad(self, loss_scale=1.0):
        self.go = self._buf("go", self.o.shape)
        M_.keypoint_loss(self.o, self.tg, self.loss, self.go, self.loss_ws, loss_scale, self.weight)
        return self.loss

    def backward(self):
        """Returns d(loss)/d(pooled) bf16 [R,14,14,C]."""
        d_d4 = dense.pixel_shuffle2(self.go, self._buf("d_d4", self.d4.shape), inverse=True)      # no ReLU behind the deconv
        x = self.acts[-1]
        self.deconv.backward_weight(x, d_d4)
        g = self.deconv.backward_data(d_d4, x.shape, relu_mask=self.tower.out_mask, out=self._buf("d_tower", x.shape))
        return self.tower.backward(g, self._buf)
