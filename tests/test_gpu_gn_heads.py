"""GroupNorm heads: the 4conv1fc box head and the GN mask head (and, for the layer chain without GN, the MaskIoU head's
tower and FC trunk) against a torch-CPU fp64 autograd restatement, and the
assembled models (step, gradients, eager / grouped / replayed agreement, checkpoints, predict, defaults). Small images,
as tests/test_gpu_dpool_model.py.

Head parity tolerance. The form is that of tests/test_gpu_dense.py::test_layer_gradients_vs_torch_fp32: rms-relative
error per tensor, 1e-3 for a single layer. These heads store 9 (box) / 11 (mask) bf16 activations and as many bf16
gradients in a row, so the bound per tensor is measured, not chosen: the same fp64 graph is run once more with every
stored activation and every stored gradient rounded to bf16 (what the kernels store), its rms-relative error against the
unrounded fp64 run is the error bf16 storage alone causes, and the bound is max(1e-3, 2 x that). Both figures are
printed per tensor. Measured on an MI355X: forward outputs, emulation 1.7e-3 (mask) / 5.0e-3 (box), kernels 1.7e-3 /
5.1e-3; last-layer weights 4.9e-3 for both; the gradients further down (d_pooled, conv weights, gamma / beta) emulation
5.2e-2 .. 1.09e-1, kernels 5.1e-2 .. 1.10e-1, i.e. the kernels are within 1.07x of what bf16 storage alone costs (the
inputs are white noise, so ReLU masks flipped by a rounded activation carry whole gradient elements)."""
import numpy as np
import pytest

from conftest import synth_gt

pytestmark = pytest.mark.gpu


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / (np.sqrt(np.mean(ref ** 2)) + 1e-30))


def _round_fn():
    import torch

    class RoundBF16(torch.autograd.Function):
        """bf16 storage of an activation (forward) and of the gradient arriving at it (backward)."""
        @staticmethod
        def forward(ctx, x):
            return x.to(torch.bfloat16).to(torch.float64)

        @staticmethod
        def backward(ctx, g):
            return g.to(torch.bfloat16).to(torch.float64)
    return RoundBF16.apply


def _standalone(head_cls, **kw):
    """A head on an arena of its own, parameters materialised, gamma / beta / biases randomised."""
    import torch
    from mxdetection_amd.models.utils.layers import ParamArena, Workspace
    arena, ws = ParamArena("cuda"), Workspace("cuda")
    gen = torch.Generator().manual_seed(3)
    head = head_cls(arena=arena, ws=ws, device="cuda", gen=gen, **kw)
    arena.finalize()
    for l in head.layers() + head.norm_layers():
        l.materialize()
    g = torch.Generator().manual_seed(4)
    for n in head.norm_layers():
        n.gamma.copy_((1.0 + 0.5 * torch.randn(n.C, generator=g)).cuda())
        n.beta.copy_((0.3 * torch.randn(n.C, generator=g)).cuda())
    for l in head.layers():
        if l.train_bias:
            b = 0.1 * torch.randn(l.cout, generator=g)
            b[l.cout_real:] = 0
            arena.view(l.bi, "w").copy_(b.cuda())
    arena.refresh_bf16()
    for l in head.layers():
        l.refresh_transposed()
    return head, arena, ws


def _w(arena, l):
    """fp64 CPU filter as the kernels see it (bf16 working copy), OIHW."""
    return arena.view(l.wi, "wb").double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)


def _b(arena, l):
    return arena.view(l.bi, "w").double().cpu().clone().requires_grad_(True)


def _trunk(x, convs, gns, G, rnd):
    import torch
    F = torch.nn.functional
    for (w, b), (ga, be) in zip(convs, gns):
        x = rnd(F.conv2d(x, w, b, padding=1))
        x = rnd(torch.relu(F.group_norm(x, G, ga, be, 1e-5)))
    return x


def _compare(names, got, ref, emu):
    worst = 0.0
    for name in names:
        e, k = _rel(emu[name], ref[name]), _rel(got[name], ref[name])
        bound = max(1e-3, 2.0 * e)
        print("%-22s emulation %.3e  kernels %.3e  bound %.3e" % (name, e, k, bound))
        worst = max(worst, k / bound)
        assert k <= bound, (name, k, bound)
    return worst


def test_gn_box_head_matches_fp64_autograd(hip):
    import torch
    from mxdetection_amd.models.bbox_heads import ConvFCBBoxHead
    torch.set_num_threads(16)
    R, C, G = 64, 256, 32
    head, arena, ws = _standalone(ConvFCBBoxHead, in_features=7 * 7 * C, norm="gn", gn_groups=G, rois_per_image=R)
    head.plan(1)
    ws.get()
    g = torch.Generator().manual_seed(5)
    pooled = torch.randn((R, 7, 7, C), generator=g).to(torch.bfloat16)
    go = torch.randn((R, 1, 1, head.ld), generator=g).to(torch.bfloat16)
    go[..., head.nc + head.reg_dim:] = 0
    o = head.forward(pooled.cuda())
    head.go = go.cuda()
    dpool = head.backward()
    torch.cuda.synchronize()
    got = {"out": o.float().cpu().numpy().reshape(R, -1), "d_pooled": dpool.float().cpu().numpy()}
    for l in head.layers():
        got[l.name + ".weight"] = arena.view(l.wi, "g").cpu().numpy()
        if l.train_bias:
            got[l.name + ".bias"] = arena.view(l.bi, "g").cpu().numpy()
    for n in head.norm_layers():
        got[n.name + ".gamma"] = arena.view(n.gi, "g").cpu().numpy()
        got[n.name + ".beta"] = arena.view(n.bi, "g").cpu().numpy()

    def run(rnd):
        x = pooled.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        convs = [(_w(arena, c), None) for c in head.convs]
        gns = [(n.gamma.double().cpu().clone().requires_grad_(True), n.beta.double().cpu().clone().requires_grad_(True))
               for n in head.norms]
        w1, b1, wo, bo = _w(arena, head.fc1), _b(arena, head.fc1), _w(arena, head.fc_out), _b(arena, head.fc_out)
        t = _trunk(x, convs, gns, G, rnd).permute(0, 2, 3, 1).reshape(R, -1)
        h1 = rnd(torch.relu(t @ w1.reshape(w1.shape[0], -1).t() + b1))
        out = rnd(h1 @ wo.reshape(wo.shape[0], -1).t() + bo)
        out.backward(go.double().reshape(R, -1))
        res = {"out": out.detach().numpy(), "d_pooled": rnd(x.grad).permute(0, 2, 3, 1).numpy(),
               "bbox.fc1.weight": w1.grad.permute(0, 2, 3, 1).numpy(), "bbox.fc1.bias": b1.grad.numpy(),
               "bbox.fc_out.weight": wo.grad.permute(0, 2, 3, 1).numpy(), "bbox.fc_out.bias": bo.grad.numpy()}
        for i, ((w, _), (ga, be)) in enumerate(zip(convs, gns)):
            res["bbox.conv%d.weight" % i] = w.grad.permute(0, 2, 3, 1).numpy()
            res["bbox.conv%d_gn.gamma" % i], res["bbox.conv%d_gn.beta" % i] = ga.grad.numpy(), be.grad.numpy()
        return res
    # the FC weight is stored [O,1,1,(H,W,C)]: as OIHW [O,(HWC),1,1] -> permute back gives [O,1,1,HWC]: same flatten
    ref, emu = run(lambda t: t), run(_round_fn())
    assert set(got) == set(ref)
    _compare(sorted(ref), got, ref, emu)


def test_gn_mask_head_matches_fp64_autograd(hip):
    import torch
    from mxdetection_amd.models.mask_heads import FCNMaskHead
    torch.set_num_threads(16)
    R, C, G = 16, 256, 32
    head, arena, ws = _standalone(FCNMaskHead, channels=C, norm="gn", gn_groups=G, rois_per_image=R)
    head.plan(1)
    ws.get()
    g = torch.Generator().manual_seed(6)
    pooled = torch.randn((R, 14, 14, C), generator=g).to(torch.bfloat16)
    go = torch.randn((R, 28, 28, head.cpad), generator=g).to(torch.bfloat16)
    go[..., head.nc - 1:] = 0
    o = head.forward(pooled.cuda())
    head.go = go.cuda()
    dpool = head.backward()
    torch.cuda.synchronize()
    got = {"out": o.float().cpu().numpy(), "d_pooled": dpool.float().cpu().numpy()}
    for l in head.layers():
        got[l.name + ".weight"] = arena.view(l.wi, "g").cpu().numpy()
        if l.train_bias:
            got[l.name + ".bias"] = arena.view(l.bi, "g").cpu().numpy()
    for n in head.norm_layers():
        got[n.name + ".gamma"] = arena.view(n.gi, "g").cpu().numpy()
        got[n.name + ".beta"] = arena.view(n.bi, "g").cpu().numpy()

    def run(rnd):
        F = torch.nn.functional
        x = pooled.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        convs = [(_w(arena, c), None) for c in head.convs]
        gns = [(n.gamma.double().cpu().clone().requires_grad_(True), n.beta.double().cpu().clone().requires_grad_(True))
               for n in head.norms]
        wd, bd, wl, bl = _w(arena, head.deconv), _b(arena, head.deconv), _w(arena, head.logits), _b(arena, head.logits)
        t = _trunk(x, convs, gns, G, rnd)
        d4 = rnd(torch.relu(F.conv2d(t, wd, bd)))                         # [R, 4C, 14, 14], channel = (dy*2+dx)*C + c
        up = d4.reshape(R, 2, 2, C, 14, 14).permute(0, 3, 4, 1, 5, 2).reshape(R, C, 28, 28)
        out = rnd(F.conv2d(up, wl, bl))
        out.backward(go.double().permute(0, 3, 1, 2))
        res = {"out": out.detach().permute(0, 2, 3, 1).numpy(), "d_pooled": rnd(x.grad).permute(0, 2, 3, 1).numpy(),
               "mask.deconv.weight": wd.grad.permute(0, 2, 3, 1).numpy(), "mask.deconv.bias": bd.grad.numpy(),
               "mask.logits.weight": wl.grad.permute(0, 2, 3, 1).numpy(), "mask.logits.bias": bl.grad.numpy()}
        for i, ((w, _), (ga, be)) in enumerate(zip(convs, gns)):
            res["mask.conv%d.weight" % i] = w.grad.permute(0, 2, 3, 1).numpy()
            res["mask.conv%d_gn.gamma" % i], res["mask.conv%d_gn.beta" % i] = ga.grad.numpy(), be.grad.numpy()
        return res
    ref, emu = run(lambda t: t), run(_round_fn())
    assert set(got) == set(ref)
    _compare(sorted(ref), got, ref, emu)


@pytest.mark.parametrize("R,fc_dim", [(8, 64), (64, None)])
def test_maskiou_tower_and_fcs_match_fp64_autograd(hip, R, fc_dim):
    """The chain without GN in the MaskIoU head's shape: a wider layer 0 (320 -> C), a strided last conv, biases, then the
    FC trunk through a `view`, with fc1's ReLU mask taken from the tower's last activation. 64 channels are the fewest the
    dense kernels take (forward Cin % 64, data gradient Cout % 64), fc_dim 64 likewise. R = 8 runs fc1's plain kernel,
    R = 64 at the default fc_dim its split-K route. The graph starts at the head's assembled input (core.mask.maskiou_input
    has tests of its own); the input gradient is compared on the feature channels [0, C), all the caller reads.
    Measured on an MI355X: outputs, emulation 1.8e-3, kernels 1.8e-3; gradients, emulation 1.8e-3 .. 1.0e-1, kernels within
    1.07x of the emulation on every tensor (bound: 2x)."""
    import torch
    from mxdetection_amd.models.mask_heads import MaskIoUHead
    torch.set_num_threads(16)
    C = 64
    head, arena, ws = _standalone(MaskIoUHead, channels=C, rois_per_image=R, **({} if fc_dim is None else {"fc_dim": fc_dim}))
    head.plan(1)
    ws.get()
    g = torch.Generator().manual_seed(7)
    mpooled = torch.randn((R, 14, 14, C), generator=g).to(torch.bfloat16)
    logits = torch.randn((R, 28, 28, 128), generator=g).to(torch.bfloat16)
    cls = torch.randint(1, head.nc, (R,), generator=g).to(torch.int32)
    go = torch.randn((R, 1, 1, head.ld), generator=g).to(torch.bfloat16)
    go[..., head.nc - 1:] = 0
    o = head.forward(mpooled.cuda(), logits.cuda(), cls.cuda())
    head.go = go.cuda()
    d_in = head.backward()
    torch.cuda.synchronize()
    x_in = head.acts[0].cpu()
    assert tuple(x_in.shape) == (R, 14, 14, head.cin) and tuple(d_in.shape) == tuple(x_in.shape)
    assert torch.equal(x_in[..., :C], mpooled) and not x_in[..., C + 1:].any()
    got = {"out": o.float().cpu().numpy().reshape(R, -1), "d_in": d_in[..., :C].float().cpu().numpy()}
    for l in head.layers():
        got[l.name + ".weight"] = arena.view(l.wi, "g").cpu().numpy()
        got[l.name + ".bias"] = arena.view(l.bi, "g").cpu().numpy()

    def run(rnd):
        F = torch.nn.functional
        x = x_in.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        params = {l.name: (_w(arena, l), _b(arena, l)) for l in head.layers()}
        t = x
        for c in head.convs:
            w, b = params[c.name]
            t = rnd(torch.relu(F.conv2d(t, w, b, stride=c.stride, padding=1)))
        t = t.permute(0, 2, 3, 1).reshape(R, -1)           # the head's view: (H, W, C) flattened
        for fc, relu in ((head.fc1, True), (head.fc2, True), (head.fc_out, False)):
            w, b = params[fc.name]
            t = t @ w.reshape(w.shape[0], -1).t() + b
            t = rnd(torch.relu(t) if relu else t)
        t.backward(go.double().reshape(R, -1))
        res = {"out": t.detach().numpy(), "d_in": rnd(x.grad).permute(0, 2, 3, 1)[..., :C].numpy()}
        for name, (w, b) in params.items():
            res[name + ".weight"], res[name + ".bias"] = w.grad.permute(0, 2, 3, 1).numpy(), b.grad.numpy()
        return res
    ref, emu = run(lambda t: t), run(_round_fn())
    assert set(got) == set(ref) and len(ref) == 2 + 2 * 7
    _compare(sorted(ref), got, ref, emu)


# ---- assembled models ----

def _inputs(N, H, W, seed=0, masks=False):
    import torch
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(1234 + seed)
    image = torch.randn((N, 3, H, W), generator=g).cuda()
    gt_np = synth_gt(rng, N, 16, H, W - 5)
    gt = torch.from_numpy(gt_np).cuda()
    im_info = torch.tensor([[H, W - 5, 1.0]] * N, dtype=torch.float32).cuda()
    if not masks:
        return image, gt, im_info
    gm = np.zeros((N, 16, H, W), np.uint8)
    for n in range(N):
        for k in range(16):
            if gt_np[n, k, 4] > 0:
                x1, y1, x2, y2 = [int(v) for v in gt_np[n, k, :4]]
                gm[n, k, y1:y2 + 1, x1:x2 + 1] = 1
    return image, gt, im_info, torch.from_numpy(gm).cuda()


KW = dict(seed=7, pre_nms_top_n=1000, post_nms_top_n=1000, bbox_head="4conv1fc", head_norm="gn")


@pytest.mark.parametrize("with_mask", [False, True])
def test_gn_model_step_is_finite_with_gradients_everywhere(hip, with_mask):
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 2, 256, 320
    inp = _inputs(N, H, W, seed=1, masks=with_mask)
    m = FasterRCNN("cuda", with_mask=with_mask, **KW)
    names = [e[0] for e in m.arena.entries]
    want = ["bbox.conv%d_gn.%s" % (i, p) for i in range(4) for p in ("gamma", "beta")]
    if with_mask:
        want += ["mask.conv%d_gn.%s" % (i, p) for i in range(4) for p in ("gamma", "beta")]
    assert set(want) <= set(names) and "bbox.fc2.weight" not in names and "bbox.conv0.bias" not in names
    losses = torch.cat(m.forward_backward(*inp[:3], step=2, gt_masks=inp[3] if with_mask else None)).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(m.arena.g).all()
    grads = m.export_grads()
    for name in want + ["bbox.conv%d.weight" % i for i in range(4)] + ["bbox.fc1.weight"]:
        assert grads[name].abs().sum().item() > 0, name
    fo = m.bbox_head.fc_out
    assert not m.arena.view(fo.wi, "g")[fo.cout_real:].any() and not m.arena.view(fo.bi, "g")[fo.cout_real:].any()
    if with_mask:
        lo = m.mask_head.logits
        assert not m.arena.view(lo.wi, "g")[lo.cout_real:].any()


def test_gn_model_grouped_replayed_and_eager_steps_agree(hip):
    """Eager launches, grouped weight gradients on the side stream and the replayed hipGraph step give the same losses
    and gradient arena (bounds of tests/test_gpu_dpool_model.py); two replayed steps move the GN parameters, i.e. the
    head bucket's update ran behind the GN backward kernels that write its gradients."""
    import torch
    from mxdetection_amd.models import FasterRCNN
    N, H, W = 2, 256, 320
    image, gt, im_info, gm = _inputs(N, H, W, seed=2, masks=True)
    ref = FasterRCNN("cuda", with_mask=True, **KW)
    l_ref = torch.cat(ref.forward_backward(image, gt, im_info, step=4, image_offset=0, gt_masks=gm)).clone()
    g_ref = ref.arena.g.clone()
    m = FasterRCNN("cuda", with_mask=True, **KW)
    m.enable_wgrad_stream()
    m.enable_branch_stream()
    m.enable_grouped_wgrad()
    l_side = torch.cat(m.forward_backward(image, gt, im_info, step=4, image_offset=0, gt_masks=gm)).clone()
    m.ws.join()
    torch.cuda.synchronize()
    assert torch.equal(l_ref, l_side)
    denom = g_ref.abs().max().item()
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom
    for n in m.norm_layers:
        for idx in (n.gi, n.bi):
            a, r = m.arena.view(idx, "g"), ref.arena.view(idx, "g")
            assert r.abs().sum().item() > 0 and torch.equal(a, r), n.name          # deterministic kernels: bit-equal
    m.capture(image, gt, im_info, lr=0.0, image_offset=0, warmup=1, gt_masks=gm)
    l_graph = torch.cat(m.replay(image, gt, im_info, 4, gt_masks=gm)).clone()
    torch.cuda.synchronize()
    assert torch.allclose(l_ref, l_graph, rtol=1e-4, atol=1e-5), (l_ref, l_graph)
    assert (g_ref - m.arena.g).abs().max().item() <= 1e-3 * denom
    before = [m.arena.view(n.gi, "w").clone() for n in m.norm_layers] + [m.arena.view(n.bi, "w").clone() for n in m.norm_layers]
    assert all(bool((b == 1).all()) for b in before[:len(m.norm_layers)])          # lr = 0 so far: still the initial state
    m.replay(image, gt, im_info, 5, gt_masks=gm, lr=0.01)
    m.replay(image, gt, im_info, 6, gt_masks=gm, lr=0.01)
    torch.cuda.synchronize()
    after = [m.arena.view(n.gi, "w") for n in m.norm_layers] + [m.arena.view(n.bi, "w") for n in m.norm_layers]
    for b, a in zip(before, after):
        assert torch.isfinite(a).all() and not torch.equal(a, b)


def test_gn_checkpoint_round_trip_and_predict(hip, tmp_path):
    import torch
    from mxdetection_amd.models import FasterRCNN
    from mxdetection_amd.utils import load_params
    N, H, W = 1, 192, 256
    image, gt, im_info, gm = _inputs(N, H, W, seed=4, masks=True)
    kw = dict(KW, pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128, with_mask=True)
    a = FasterRCNN("cuda", **kw)
    a.train_step(image, gt, im_info, step=0, lr=0.01, gt_masks=gm)
    a.train_step(image, gt, im_info, step=1, lr=0.01, gt_masks=gm)
    fn = str(tmp_path / "gn-0001.params")
    a.save_checkpoint(fn)
    blob = load_params(fn)
    assert blob["arg:bbox.conv2_gn.gamma"].shape == (256,) and blob["arg:mask.conv0_gn.beta"].shape == (256,)
    assert blob["aux:momentum:bbox.conv2_gn.gamma"].shape == (256,)
    assert blob["arg:bbox.conv1.weight"].shape == (256, 256, 3, 3) and "arg:bbox.conv1.bias" not in blob
    assert blob["arg:bbox.fc1.weight"].shape == (1024, 12544)
    b = FasterRCNN("cuda", **dict(kw, seed=11))
    assert b.load_checkpoint(fn) == []
    for (na, _, ta, _), (nb, _, tb, _) in zip(a._named_tensors(), b._named_tensors()):
        assert na == nb and torch.equal(ta, tb), na
    assert torch.equal(a.arena.w, b.arena.w) and torch.equal(a.arena.m, b.arena.m)
    assert set(a.export_params()) == set(b.export_params()) and "bbox.conv0_gn.gamma" in a.export_params()
    dets, num, masks = b.predict(image, im_info, with_masks=True)
    torch.cuda.synchronize()
    assert dets.shape == (N, 100, 6) and torch.isfinite(dets).all() and 0 <= int(num[0]) <= 100
    assert masks.shape == (N, 100, H, W) and masks.dtype == torch.uint8 and int(masks.max()) <= 1
    k = int(num[0])
    assert bool((dets[0, k:, 5] == -1).all()) and not masks[0, k:].any()


def test_default_model_has_todays_parameters(hip):
    from mxdetection_amd.models import FasterRCNN
    m = FasterRCNN("cuda", pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128)
    assert m.norm_layers == []
    ent = [(e[0], e[1]) for e in m.arena.entries]
    assert ent[:6] == [("bbox.fc_out.weight", (448, 1, 1, 1024)), ("bbox.fc_out.bias", (448,)),
                       ("bbox.fc2.weight", (1024, 1, 1, 1024)), ("bbox.fc2.bias", (1024,)),
                       ("bbox.fc1.weight", (1024, 1, 1, 12544)), ("bbox.fc1.bias", (1024,))]
    assert not [n for n, _ in ent if "gn" in n or "bbox.conv" in n]
    explicit = FasterRCNN("cuda", pre_nms_top_n=600, post_nms_top_n=300, rois_per_image=128, bbox_head="2fc",
                          head_norm="none", gn_groups=32)
    assert [(e[0], e[1], e[2]) for e in explicit.arena.entries] == [(e[0], e[1], e[2]) for e in m.arena.entries]
    import torch
    assert torch.equal(explicit.arena.w, m.arena.w)
