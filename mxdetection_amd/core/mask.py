"""core/mask (/root/reference/README.md:18): mask-target generation and the mask loss for Mask R-CNN."""
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr


def mask_target(rois, matched_gt, labels, gt_masks, size=28, out=None):
    """rois [R,5] f32, matched_gt/labels [R] i32, gt_masks [N,G,H,W] u8 -> (targets [R,S,S] u8, cls [R] i32)."""
    lib = _lib.load()
    R = rois.shape[0]
    N, G, H, W = gt_masks.shape
    if out is None:
        tg = torch.empty((R, size, size), dtype=torch.uint8, device=rois.device)
        cls = torch.empty((R,), dtype=torch.int32, device=rois.device)
    else:
        tg, cls = out
    check(lib.mxdet_mask_target(ptr(rois), ptr(matched_gt), ptr(labels), ptr(gt_masks), R, G, H, W, size, ptr(tg),
                                ptr(cls), stream_ptr()), "mask_target")
    return tg, cls


def mask_loss_workspace(R, S, device):
    return torch.empty((_lib.load().mxdet_mask_loss_workspace_bytes(R, S),), dtype=torch.uint8, device=device)


def mask_loss(logits, cls, targets, loss_out, grad, workspace, loss_scale=1.0):
    """logits/grad bf16 [R,S,S,Cpad]; cls [R] i32; targets [R,S,S] u8; loss_out f32[1]."""
    lib = _lib.load()
    R, S, _, Cpad = logits.shape
    check(lib.mxdet_mask_loss(ptr(logits), ptr(cls), ptr(targets), R, S, Cpad, loss_scale, ptr(loss_out), ptr(grad),
                              ptr(workspace), workspace.numel(), stream_ptr()), "mask_loss")
    return loss_out


MASKIOU_CIN = 320       # MaskIoU head input channels: 256 features + the mask channel, padded to a multiple of 64


def maskiou_target_workspace_bytes(N, G):
    return _lib.load().mxdet_maskiou_target_workspace_bytes(N, G)


def maskiou_target_workspace(N, G, device):
    return torch.empty((maskiou_target_workspace_bytes(N, G),), dtype=torch.uint8, device=device)


def maskiou_target(rois, matched_gt, cls, gt_boxes, gt_masks, logits, targets, out=None, workspace=None):
    """Mask Scoring R-CNN's regression target (mxdet_maskiou_target): rois [R,5] f32, matched_gt / cls [R] i32 (cls as
    mask_target writes it), gt_boxes [N,G_boxes >= G,5] f32, gt_masks [N,G,H,W] u8, logits bf16 [R,S,S,Cpad], targets u8 [R,S,S]
    -> f32 [R]."""
    lib = _lib.load()
    R, S, _, Cpad = logits.shape
    N, G, H, W = gt_masks.shape
    if workspace is None:
        workspace = maskiou_target_workspace(N, G, rois.device)
    if out is None:
        out = torch.empty((R,), dtype=torch.float32, device=rois.device)
    check(lib.mxdet_maskiou_target(ptr(rois), ptr(matched_gt), ptr(cls), ptr(gt_boxes), ptr(gt_masks), ptr(logits),
                                   ptr(targets), R, N, G, gt_boxes.shape[1], H, W, S, Cpad, ptr(out), ptr(workspace), workspace.numel(),
                                   stream_ptr()), "maskiou_target")
    return out


def maskiou_input(mpooled, logits, cls, out=None, channels=MASKIOU_CIN):
    """mpooled bf16 [R,h,h,C], logits bf16 [R,2h,2h,Cpad], cls [R] i32 -> bf16 [R,h,h,channels]: the features, the 2x2
    max-pooled mask probability of the class channel, zeros (mxdet_maskiou_input)."""
    lib = _lib.load()
    R, h, _, C = mpooled.shape
    S, Cpad = logits.shape[1], logits.shape[3]
    assert S == 2 * h and logits.shape[0] == R
    if out is None:
        out = torch.empty((R, h, h, channels), dtype=torch.bfloat16, device=mpooled.device)
    check(lib.mxdet_maskiou_input(ptr(mpooled), ptr(logits), ptr(cls), R, S, C, Cpad, out.shape[3], ptr(out), stream_ptr()),
          "maskiou_input")
    return out


def maskiou_input_bwd(d_in, d_mpooled):
    """d_mpooled bf16 [R,h,h,C] += channels [0,C) of d_in bf16 [R,h,h,Ctot], one bf16 rounding (in place)."""
    lib = _lib.load()
    R, h, w, C = d_mpooled.shape
    check(lib.mxdet_maskiou_input_bwd(ptr(d_in), R * h * w, C, d_in.shape[3], ptr(d_mpooled), stream_ptr()),
          "maskiou_input_bwd")
    return d_mpooled


def maskiou_loss(pred, cls, targets, loss_out, grad, loss_scale=1.0, weight=1.0):
    """pred / grad bf16 [R,ld]; cls [R] i32; targets f32 [R]; loss_out f32[1] (mxdet_maskiou_loss)."""
    lib = _lib.load()
    R, ld = pred.shape
    check(lib.mxdet_maskiou_loss(ptr(pred), ptr(cls), ptr(targets), R, ld, loss_scale, weight, ptr(loss_out), ptr(grad),
                                 stream_ptr()), "maskiou_loss")
    return loss_out


def maskiou_score(dets, pred, out=None):
    """dets [R,6] f32 (x1,y1,x2,y2,score,class), pred bf16 [R,ld] -> mask scores f32 [R] (mxdet_maskiou_score)."""
    lib = _lib.load()
    R, ld = pred.shape
    if out is None:
        out = torch.empty((R,), dtype=torch.float32, device=dets.device)
    check(lib.mxdet_maskiou_score(ptr(dets), ptr(pred), R, ld, ptr(out), stream_ptr()), "maskiou_score")
    return out


def keypoint_target(rois, matched_gt, labels, gt_keypoints, size_in=28, out=None):
    """Keypoint R-CNN's heatmap target (mxdet_keypoint_target): rois [R,5] f32, matched_gt / labels [R] i32, gt_keypoints
    [N,G,K,3] f32 (x, y, v) -> int32 [R,K]: the linear index into the (2*size_in)^2 upsampled map, -1 = not trained."""
    lib = _lib.load()
    R = rois.shape[0]
    N, G, K, _ = gt_keypoints.shape
    if out is None:
        out = torch.empty((R, K), dtype=torch.int32, device=rois.device)
    check(lib.mxdet_keypoint_target(ptr(rois), ptr(matched_gt), ptr(labels), ptr(gt_keypoints), R, N, G, K, size_in, ptr(out),
                                    stream_ptr()), "keypoint_target")
    return out


def keypoint_loss_workspace(R, device):
    return torch.empty((_lib.load().mxdet_keypoint_loss_workspace_bytes(R),), dtype=torch.uint8, device=device)


def keypoint_loss(logits, targets, loss_out, grad, workspace, loss_scale=1.0, weight=1.0, num_keypoints=None):
    """logits / grad bf16 [R,S_in,S_in,Kpad]; targets int32 [R,K]; loss_out f32[1] (mxdet_keypoint_loss): softmax
    cross-entropy over the x2 upsampled map of every valid (roi, keypoint), normalised by their number."""
    lib = _lib.load()
    R, S_in, _, Kpad = logits.shape
    K = targets.shape[1] if num_keypoints is None else num_keypoints
    check(lib.mxdet_keypoint_loss(ptr(logits), ptr(targets), R, S_in, Kpad, K, loss_scale, weight, ptr(loss_out), ptr(grad),
                                  ptr(workspace), workspace.numel(), stream_ptr()), "keypoint_loss")
    return loss_out


def keypoint_decode(logits, dets, num_keypoints, out=None):
    """logits bf16 [R,S_in,S_in,Kpad], dets [R,6] f32 (x1,y1,x2,y2,score,class) -> f32 [R,K,3] = (x, y, score): the argmax of
    the x2 upsampled map of each keypoint channel, placed in the box (mxdet_keypoint_decode); zeros on padding rows."""
    lib = _lib.load()
    R, S_in, _, Kpad = logits.shape
    if out is None:
        out = torch.empty((R, num_keypoints, 3), dtype=torch.float32, device=logits.device)
    check(lib.mxdet_keypoint_decode(ptr(logits), ptr(dets), R, S_in, Kpad, num_keypoints, ptr(out), stream_ptr()),
          "keypoint_decode")
    return out


def mask_paste(logits, dets, H, W, thresh=0.5, out=None, workspace=None):
    """Inference paste-back: logits bf16 [R,S,S,Cpad], dets [R,6] f32 (x1,y1,x2,y2,score,class) in the output frame
    -> full-frame instance masks [R,H,W] u8 (mxdet_mask_paste)."""
    lib = _lib.load()
    R, S, _, Cpad = logits.shape
    need = lib.mxdet_mask_paste_workspace_bytes(R, S)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((need,), dtype=torch.uint8, device=logits.device)
    if out is None:
        out = torch.empty((R, H, W), dtype=torch.uint8, device=logits.device)
    check(lib.mxdet_mask_paste(ptr(logits), ptr(dets), R, S, Cpad, H, W, thresh, ptr(out), ptr(workspace), workspace.numel(),
                               stream_ptr()), "mask_paste")
    return out
