"""Every dense conv / weight-gradient tile route and geometry on the GPU against fp64 (case tables and the proof of which
route each case takes: tests/test_conv_routes_cpu.py).

Reference: torch.float64 on the CPU of the same bf16-exact operands (a matrix product for 1x1 layers), plus the C oracle
(double accumulation) on the small square-filter cases. Tolerances are the project's: bf16 outputs `_close` of
test_gpu_dense.py on every element; fp32 weight / bias gradients max|got - ref| <= 2e-4 rms(ref) + 1e-5 max|ref|. Without a
tolerance: masked / unreachable elements are exactly zero (or exactly the residual), outputs are pre-filled with NaN or a
sentinel, relu_bits equal the stored values bit for bit, and within one K-loop flavour every tile gives the bits of the
64x64 tile (an element's reduction order -- channel slices, taps inside a slice, two 32-deep halves -- does not depend on
the tile). The parity-grouped stride-2 data gradient has a flavour of its own (only the taps of a row's parity class): its
64x128 tile is compared with its 64x64 tile (PAR64 high); at <= 64 columns it has the 128x64 tile only, checked against
fp64. The grouped weight gradient runs the nine-item mix under every launch-time choice (ring depths, mixed grid, split
depth) and as three separately issued parts on two streams.
"""
import numpy as np
import pytest

import test_conv_routes_cpu as R
from test_gpu_dense import _close

pytestmark = pytest.mark.gpu
_REF = {}


def _rand(seed, shape, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def _nhwc64(t):
    return t.double().permute(0, 3, 1, 2)


def _key(c):
    return (c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KW"], c["s"], c["p"])


def _operands(c, red_first=True):
    """x [N,H,W,Cin], w [Cout,KH,KW,Cin], dy [N,Ho,Wo,Cout] (bf16, CPU), seeded by the case's shape."""
    Ho, Wo = R.out_hw(c)
    key = _key(c)
    seed = hash(key) % (2 ** 31)
    fan = c["KH"] * c["KW"] * (c["Cin"] if red_first else c["Cout"])
    x = _rand(seed, (c["N"], c["H"], c["W"], c["Cin"]))
    w = _rand(seed + 1, (c["Cout"], c["KH"], c["KW"], c["Cin"]), (2.0 / fan) ** 0.5)
    dy = _rand(seed + 2, (c["N"], Ho, Wo, c["Cout"]))
    return key, x, w, dy


def _ref_fwd(c, x, w):
    import torch
    k = ("fwd",) + _key(c)
    if k not in _REF:
        if (c["KH"], c["KW"], c["s"], c["p"]) == (1, 1, 1, 0):
            y = (x.double().reshape(-1, c["Cin"]) @ w.double().reshape(c["Cout"], -1).t()).reshape(x.shape[:3] + (c["Cout"],))
        else:
            y = torch.nn.functional.conv2d(_nhwc64(x), _nhwc64(w), stride=c["s"], padding=c["p"]).permute(0, 2, 3, 1)
        _REF.clear()                                   # one big reference at a time
        _REF[k] = y.contiguous().numpy()
    return _REF[k]


def _ref_dgrad(c, dy, w):
    import torch
    k = ("dgrad",) + _key(c)
    if k not in _REF:
        shape = (c["N"], c["Cin"], c["H"], c["W"])
        if (c["KH"], c["KW"], c["s"], c["p"]) == (1, 1, 1, 0):
            dx = (dy.double().reshape(-1, c["Cout"]) @ w.double().reshape(c["Cout"], -1)).reshape(c["N"], c["H"], c["W"], c["Cin"])
        else:
            dx = torch.nn.grad.conv2d_input(shape, _nhwc64(w), _nhwc64(dy), stride=c["s"], padding=c["p"]).permute(0, 2, 3, 1)
        _REF.clear()
        _REF[k] = dx.contiguous().numpy()
    return _REF[k]


def _np(t):
    return t.float().cpu().numpy()


def _nan_like(shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device="cuda")


def _pack_bits(y):
    import torch
    b = (y.reshape(y.shape[:-1] + (y.shape[-1] // 8, 8)) > 0).to(torch.int32)
    return (b * (2 ** torch.arange(8, device=y.device, dtype=torch.int32))).sum(-1).to(torch.uint8)


def _fwd_variants(c, x, w, steer_args):
    """Run every forward epilogue under one steering; returns {variant: tensors}."""
    import torch
    from mxdetection_amd.ops import dense
    Ho, Wo = R.out_hw(c)
    shape = (c["N"], Ho, Wo, c["Cout"])
    seed = 7 + c["Cout"]
    bias = torch.randn((c["Cout"],), generator=torch.Generator().manual_seed(seed)).cuda()
    res = _rand(seed + 1, shape).cuda()
    coarse = _rand(seed + 2, (c["N"], (Ho + 1) // 2, (Wo + 1) // 2, c["Cout"])).cuda()
    xd, wd = x.cuda(), w.cuda()
    out = {"bias": bias, "res": res, "coarse": coarse}
    with R.steer(*steer_args):
        y, bits = _nan_like(shape), torch.full(shape[:3] + (c["Cout"] // 8,), 0xAA, dtype=torch.uint8, device="cuda")
        dense.conv2d_forward(xd, wd, bias, None, c["s"], c["p"], True, out=y, bits_out=bits)
        out["A"], out["A_bits"] = y, bits
        out["B"] = dense.conv2d_forward(xd, wd, None, res, c["s"], c["p"], False, out=_nan_like(shape))
        out["C"] = dense.conv2d_forward(xd, wd, bias, coarse, c["s"], c["p"], True, res_upsample=True, out=_nan_like(shape))
        torch.cuda.synchronize()
    return out


def _dgrad_variants(c, dy, w, steer_args):
    import torch
    from mxdetection_amd.ops import dense
    shape = (c["N"], c["H"], c["W"], c["Cin"])
    seed = 11 + c["Cin"]
    res = _rand(seed, shape).cuda()
    act = torch.relu(_rand(seed + 1, shape)).cuda()
    bits = _pack_bits(act)
    dyd = dy.cuda()
    wt = dense.filter_transpose(w.cuda())
    K = (c["KH"], c["KW"], c["s"], c["p"])
    out = {"res": res, "act": act}
    with R.steer(*steer_args):
        out["P"] = dense.conv2d_dgrad(dyd, wt, shape, *K, out=_nan_like(shape))
        out["Q"] = dense.conv2d_dgrad(dyd, wt, shape, *K, residual=res, relu_mask=act, out=_nan_like(shape))
        out["R"] = dense.conv2d_dgrad(dyd, wt, shape, *K, residual=res, relu_bits=bits, out=_nan_like(shape))
        out["S"] = dense.conv2d_dgrad(dyd, wt, shape, *K, accumulate=True, out=res.clone())
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", [c["name"] for c in R.CONV_CASES])
def test_conv_case(hip, oracle, name):
    import torch
    torch.set_num_threads(16)
    c = R.CONV_BY_NAME[name]
    recs = R.conv_records(c)
    assert [R.route_name(r) for r in recs] == c["route"]
    M, cols = R.rows_cols(c)
    small = M * cols * c["KH"] * c["KW"] * (c["Cin"] if c["kind"] == "fwd" else c["Cout"]) < 2e8 and c["KH"] == c["KW"]
    if c["kind"] == "fwd":
        _, x, w, _ = _operands(c)
        got = _fwd_variants(c, x, w, (c["tune"], c["force"]))
        ref = _ref_fwd(c, x, w)
        b, res = _np(got["bias"]).astype(np.float64), _np(got["res"]).astype(np.float64)
        up = _np(got["coarse"]).astype(np.float64)[:, np.arange(ref.shape[1]) // 2][:, :, np.arange(ref.shape[2]) // 2]
        _close(_np(got["A"]), np.maximum(ref + b, 0), name + " bias+relu")
        assert torch.equal(got["A_bits"], _pack_bits(got["A"])), name + " relu_bits != stored values"
        _close(_np(got["B"]), ref + res, name + " residual")
        _close(_np(got["C"]), np.maximum(ref + b + up, 0), name + " upsampled residual")
        if small:
            xo, wo = x.float().numpy(), w.float().numpy()
            _close(_np(got["A"]), oracle.conv2d_fwd(xo, wo, _np(got["bias"]), None, c["s"], c["p"], True), name + " vs oracle")
        keys = ("A", "A_bits", "B", "C")
        again = lambda sa: _fwd_variants(c, x, w, sa)       # noqa: E731
    else:
        _, _, w, dy = _operands(c, False)
        got = _dgrad_variants(c, dy, w, (c["tune"], c["force"]))
        ref = _ref_dgrad(c, dy, w)
        res, keep = _np(got["res"]).astype(np.float64), _np(got["act"]) > 0
        _close(_np(got["P"]), ref, name + " plain")
        _close(_np(got["Q"]), (ref + res) * keep, name + " residual + mask")
        assert torch.all(got["Q"][~(got["act"] > 0)] == 0), name + ": masked elements must be exactly zero"
        assert torch.equal(got["Q"], got["R"]), name + ": 1-bit mask != 16-bit mask"
        _close(_np(got["S"]), ref + res, name + " accumulate")
        if c["s"] > 1 and c["KH"] == 1 and c["KW"] == 1 and c["p"] == 0:
            # rows / columns no output pixel reaches: exactly zero, exactly the residual
            s = c["s"]
            dead = torch.ones(got["P"].shape[1:3], dtype=torch.bool, device="cuda")
            dead[::s, ::s] = False
            assert torch.all(got["P"][:, dead] == 0) and torch.equal(got["S"][:, dead], got["res"][:, dead])
        if small:
            _close(_np(got["P"]), oracle.conv2d_dgrad(dy.float().numpy(), w.float().numpy(), got["P"].shape, c["s"], c["p"]),
                   name + " vs oracle")
        keys = ("P", "Q", "R", "S")
        again = lambda sa: _dgrad_variants(c, dy, w, sa)    # noqa: E731
    # tile independence: the rows of each launch carry the bits of the 64x64 tile of the same K-loop flavour
    if c["route"] == [R.S64x128 + " dgrad par T0"]:
        twin = again((R.PAR_HI, 0))
        for k in keys:
            assert torch.equal(got[k], twin[k]), "%s %s: 64x128 parity tile differs from the 64x64 parity tile" % (name, k)
    if not any(r[7] for r in recs):
        base = {}
        for r in recs:
            taps, lo = r[8], r[12]
            hi = min(M, lo + r[10] * r[1])
            if taps not in base:
                base[taps] = again(({}, R.baseline_force(taps)))
            for k in keys:
                a, b_ = got[k].reshape(M, -1)[lo:hi], base[taps][k].reshape(M, -1)[lo:hi]
                assert torch.equal(a, b_), "%s %s rows [%d, %d): %d elements differ from the 64x64 tile" % (
                    name, k, lo, hi, int((a != b_).sum()))


@pytest.mark.parametrize("name", [c["name"] for c in R.SPLITK_CASES])
def test_splitk_case(hip, name):
    import torch
    from mxdetection_amd.ops import dense
    torch.set_num_threads(16)
    c = R.SPLITK_BY_NAME[name]
    assert [R.route_name(r) for r in R.conv_records(c)] == c["route"]
    _, x, w, _ = _operands(c)
    ref = _ref_fwd(c, x, w)
    shape = ref.shape
    bias = torch.randn((c["Cout"],), generator=torch.Generator().manual_seed(3)).cuda()
    res = _rand(4, shape).cuda()
    want = np.maximum(ref + _np(bias).astype(np.float64) + _np(res).astype(np.float64), 0)
    need = c["ksplit"] * ref.size * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN partials: an unwritten one shows
    with R.steer(c["tune"]):
        y = dense.conv2d_forward_splitk(x.cuda(), w.cuda(), bias, res, True, c["ksplit"], out=_nan_like(shape), workspace=ws)
        y2 = dense.conv2d_forward_splitk(x.cuda(), w.cuda(), bias, res, True, c["ksplit"], out=_nan_like(shape), workspace=ws)
        torch.cuda.synchronize()
    _close(_np(y), want, name)
    assert torch.equal(y, y2), name + ": second launch into the dirty workspace differs"


def test_chain_case_vs_fp64(hip):
    import torch
    from mxdetection_amd.ops import dense
    torch.set_num_threads(16)
    c = R.CHAIN_CASES[0]
    assert [R.route_name(r) for r in R.conv_records(c)] == c["route"]
    _, x, w, _ = _operands(c)
    N, H, W = c["N"], c["H"], c["W"]
    g = torch.Generator().manual_seed(5)
    b1, b2, b3 = (torch.randn((n,), generator=g) for n in (64, 256, 64))
    w2, w3 = _rand(6, (256, 1, 1, 64), 0.15), _rand(7, (64, 1, 1, 256), 0.08)
    res = _rand(8, (N, H, W, 256))
    y2, y3 = dense.conv2d_forward_chain(x.cuda(), w.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), res.cuda(), relu=True, relu2=True,
                                        out=_nan_like((N, H, W, 256)), w3=w3.cuda(), bias3=b3.cuda(), relu3=True,
                                        out3=_nan_like((N, H, W, 64)))
    torch.cuda.synchronize()
    # fp64 with the two roundings the launch makes (the 64-channel intermediate and y2 are bf16, as the unfused layers store them)
    mid = torch.relu(torch.from_numpy(_ref_fwd(c, x, w)) + b1.double()).to(torch.bfloat16).double()
    r2 = torch.relu(mid.reshape(-1, 64) @ w2.double().reshape(256, 64).t() + b2.double() + res.double().reshape(-1, 256))
    _close(_np(y2).reshape(-1, 256), r2.numpy(), "chain y2")
    r3 = torch.relu(y2.cpu().double().reshape(-1, 256) @ w3.double().reshape(64, 256).t() + b3.double())
    _close(_np(y3).reshape(-1, 64), r3.numpy(), "chain y3")


@pytest.mark.parametrize("name", [c["name"] for c in R.GROUP_CASES])
def test_grouped_case(hip, name):
    """Per item: fp64, and the bits of the single launch of the same tile. Item 0 carries an upsampled residual (forward) /
    residual + 16-bit mask (dgrad), item 1 relu_bits, item 2 a residual (forward) / accumulate (dgrad); the group carries a
    prefetch hint."""
    import torch
    from mxdetection_amd.ops import dense
    torch.set_num_threads(16)
    c = R.GROUP_BY_NAME[name]
    fwd = c["kind"] == "fwd"
    calls, singles, refs = [], [], []
    for i, (N, H, W, Cin, Cout, K, pad) in enumerate(R.group_items(c)):
        one = dict(kind=c["kind"], N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, s=1, p=pad)
        _, x, w, dy = _operands(one, fwd)
        col = Cout if fwd else Cin
        shape = (N, H, W, col)
        res = _rand(20 + i, shape).cuda()
        if fwd:
            bias = torch.randn((Cout,), generator=torch.Generator().manual_seed(30 + i)).cuda()
            coarse = _rand(40 + i, (N, (H + 1) // 2, (W + 1) // 2, Cout)).cuda()
            bits = torch.full((N, H, W, Cout // 8), 0xAA, dtype=torch.uint8, device="cuda") if i == 1 else None
            r_, up = (coarse, True) if i == 0 else ((None, False) if i == 1 else (res, False))
            out = _nan_like(shape)
            calls.append((x.cuda(), w.cuda(), bias, r_, 1, pad, True, up, out, bits))
            ref = _ref_fwd(one, x, w) + _np(bias).astype(np.float64)
            if i == 0:
                ref = ref + _np(coarse).astype(np.float64)[:, np.arange(H) // 2][:, :, np.arange(W) // 2]
            elif i == 2:
                ref = ref + _np(res).astype(np.float64)
            refs.append(np.maximum(ref, 0))
        else:
            act = torch.relu(_rand(50 + i, shape)).cuda()
            wt = dense.filter_transpose(w.cuda())
            ref = _ref_dgrad(one, dy, w)
            if i == 0:
                calls.append((dy.cuda(), wt, shape, K, K, 1, pad, res, act, False, _nan_like(shape)))
                refs.append((ref + _np(res).astype(np.float64)) * (_np(act) > 0))
            elif i == 1:
                calls.append((dy.cuda(), wt, shape, K, K, 1, pad, None, None, False, _nan_like(shape), _pack_bits(act)))
                refs.append(ref * (_np(act) > 0))
            else:
                calls.append((dy.cuda(), wt, shape, K, K, 1, pad, None, None, True, res.clone()))
                refs.append(ref + _np(res).astype(np.float64))
    hint = dense.mem_range(calls[0][1])
    with R.steer(c["tune"]):
        plan = dense.GroupedConv(c["kind"], calls, "cuda", hint)
        assert (plan.cfg & 3, plan.cfg >> 2) == (c["cfg"], c["tc"])
        plan.launch()
        torch.cuda.synchronize()
    taps = {0: 0, 1: 1, 2: 9}[c["tc"]]
    force = R.GROUP_TILES[c["cfg"]][2 if taps == 0 else 3]
    for i, (call, ref) in enumerate(zip(calls, refs)):
        out = call[8] if fwd else call[10]
        _close(_np(out), ref, "%s item %d" % (name, i))
        with R.steer({}, force):
            if fwd:
                x, w, bias, r_, s, pad, relu, up, _, bits = call
                b1 = None if bits is None else torch.zeros_like(bits)
                one = dense.conv2d_forward(x, w, bias, r_, s, pad, relu, up, out=_nan_like(out.shape), bits_out=b1)
                if bits is not None:
                    assert torch.equal(bits, b1) and torch.equal(bits, _pack_bits(out))
            else:
                dy, wt, shape, KH, KW, s, pad, r_, mask, acc = call[:10]
                bits = call[11] if len(call) > 11 else None
                o = _rand(20 + i, shape).cuda() if acc else _nan_like(shape)
                one = dense.conv2d_dgrad(dy, wt, shape, KH, KW, s, pad, residual=r_, relu_mask=mask, accumulate=acc, out=o, relu_bits=bits)
            torch.cuda.synchronize()
        assert torch.equal(out, one), "%s item %d: grouped launch differs from the single launch of the same tile" % (name, i)


def _wgrad_ref(c, x, dy):
    import torch
    gw = torch.nn.grad.conv2d_weight(_nhwc64(x), (c["Cout"], c["Cin"], c["KH"], c["KW"]), _nhwc64(dy), stride=c["s"], padding=c["p"])
    return gw.permute(0, 2, 3, 1).contiguous().numpy(), dy.double().reshape(-1, c["Cout"]).sum(0).numpy()


def _wgrad_close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    bound = 2e-4 * np.sqrt(np.mean(ref ** 2)) + 1e-5 * np.abs(ref).max()
    assert err <= bound, "%s: max err %.4g > %.4g" % (what, err, bound)


def _run_wgrad(c, ksplit, tune, bias=True, acc=False):
    import torch
    from mxdetection_amd.ops import dense
    torch.set_num_threads(16)
    _, x, _, dy = _operands(c)
    gw, gb = _wgrad_ref(c, x, dy)
    shape = (c["Cout"], c["KH"], c["KW"], c["Cin"])
    old_w = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    old_b = torch.randn((c["Cout"],), generator=torch.Generator().manual_seed(2)).cuda()
    SENT = 12345.0
    with R.steer(tune, 0, ksplit):
        need = dense.conv2d_wgrad_workspace_bytes((c["N"], c["H"], c["W"], c["Cin"]), c["Cout"], c["KH"], c["KW"], c["s"], c["p"])
        ws = torch.full((max(need, 256),), 0xFF, dtype=torch.uint8, device="cuda")       # NaN slabs
        outs = []
        for _ in range(2):              # the second launch finds a dirty workspace
            dw = old_w.clone() if acc else torch.full(shape, SENT, device="cuda")
            db = (old_b.clone() if acc else torch.full((c["Cout"],), SENT, device="cuda")) if bias else None
            dense.conv2d_wgrad(x.cuda(), dy.cuda(), c["KH"], c["KW"], c["s"], c["p"], dw=dw, db=db, accumulate=acc, workspace=ws)
            torch.cuda.synchronize()
            outs.append((dw, db))
    (dw, db), (dw2, db2) = outs
    assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), c["name"] + ": not reproducible over two launches"
    base_w = old_w.cpu().double().numpy() if acc else 0.0
    base_b = old_b.cpu().double().numpy() if acc else 0.0
    _wgrad_close(dw.cpu().numpy() - base_w, gw, c["name"] + " dw")
    if bias:
        _wgrad_close(db.cpu().numpy() - base_b, gb, c["name"] + " db")


@pytest.mark.parametrize("name", [c["name"] for c in R.WGRAD_CASES])
def test_wgrad_case(hip, name):
    c = R.WGRAD_BY_NAME[name]
    rc, recs, _ = R.wgrad_record(c)
    r = recs[0]
    assert rc == 0 and all(w is None or w == g for w, g in zip(c["route"], (r[1], r[2], r[5], r[6], r[7])))
    _run_wgrad(c, c["ksplit"], c["tune"], c["bias"], c["acc"])


@pytest.mark.parametrize("name", [c["name"] for c in R.GEOM_WGRAD])
def test_wgrad_geometry(hip, name):
    c = {x["name"]: x for x in R.GEOM_WGRAD}[name]
    _run_wgrad(c, 2, {})


_WGG = {}


def _wgg_data():
    """Operands (on the GPU) and fp64 references of the grouped weight-gradient mix, built once."""
    import torch
    torch.set_num_threads(16)
    if not _WGG:
        xs, dys, refs = [], [], {}
        for i, (N, H, W, Cin, Cout, K, s, p, bias, slot) in enumerate(R.WGG_ITEMS):
            c = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=K, KW=K, s=s, p=p)
            Ho, Wo = R.out_hw(c)
            x, dy = _rand(900 + 2 * i, (N, H, W, Cin)), _rand(901 + 2 * i, (N, Ho, Wo, Cout))
            gw, gb = _wgrad_ref(c, x, dy)
            w0, b0 = refs.get(slot, (0.0, 0.0))
            refs[slot] = (w0 + gw, b0 + gb)                 # items that share dw: the group sums them
            xs.append(x.cuda())
            dys.append(dy.cuda())
        _WGG.update(xs=xs, dys=dys, refs=refs)
    return _WGG


def _wgg_calls(acc=False):
    import torch
    d = _wgg_data()
    dws, dbs, calls = {}, {}, []
    for i, (N, H, W, Cin, Cout, K, s, p, bias, slot) in enumerate(R.WGG_ITEMS):
        if slot not in dws:
            dws[slot] = torch.full((Cout, K, K, Cin), 12345.0, device="cuda")
            dbs[slot] = torch.full((Cout,), 12345.0, device="cuda") if bias else None
        calls.append((d["xs"][i], d["dys"][i], K, K, s, p, dws[slot], dbs[slot], acc))
    return calls, dws, dbs


@pytest.mark.parametrize("name", list(R.WGG_CASES))
def test_grouped_wgrad_case(hip, name):
    """fp64 for every dw / db; a second launch into the dirty workspace gives the same bits; the three parts issued separately
    (tile kernels on two streams, the fold after both) give the bits of the single call."""
    import torch
    from mxdetection_amd.ops import dense
    from mxdetection_amd._lib import ptr
    tune, want, _ = R.WGG_CASES[name]
    assert tuple(R.wgg_records(name)[0][0][1:4]) == want
    refs = _wgg_data()["refs"]
    calls, dws, dbs = _wgg_calls()
    lib = hip.load()
    with R.steer(tune):
        plan = dense.GroupedWgrad(calls, "cuda")
        ws = torch.full((max(plan.workspace_bytes, 256),), 0xFF, dtype=torch.uint8, device="cuda")      # NaN slabs
        plan.launch(ws)
        torch.cuda.synchronize()
        first = {k: (dws[k].clone(), None if dbs[k] is None else dbs[k].clone()) for k in dws}
        for k in dws:                                   # sentinel again, workspace left dirty
            dws[k].fill_(12345.0)
            if dbs[k] is not None:
                dbs[k].fill_(12345.0)
        plan.launch(ws)
        torch.cuda.synchronize()
        for k in dws:
            assert torch.equal(dws[k], first[k][0]) and (dbs[k] is None or torch.equal(dbs[k], first[k][1])), "%s slot %d: not reproducible" % (name, k)
            dws[k].fill_(12345.0)
            if dbs[k] is not None:
                dbs[k].fill_(12345.0)
        ws.fill_(0xFF)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for parts, st in ((1, sa), (2, sb)):
            with torch.cuda.stream(st):
                hip.check(lib.mxdet_conv2d_wgrad_grouped_parts(ptr(plan.table), plan.n, plan.grid_wgrad, plan.grid_big, plan.grid_reduce,
                                                               parts, ptr(ws), ws.numel(), plan.workspace_bytes, hip.stream_ptr()), "parts")
        sa.synchronize()
        sb.synchronize()
        hip.check(lib.mxdet_conv2d_wgrad_grouped_parts(ptr(plan.table), plan.n, plan.grid_wgrad, plan.grid_big, plan.grid_reduce, 4,
                                                       ptr(ws), ws.numel(), plan.workspace_bytes, hip.stream_ptr()), "parts")
        torch.cuda.synchronize()
    for k in dws:
        assert torch.equal(dws[k], first[k][0]) and (dbs[k] is None or torch.equal(dbs[k], first[k][1])), "%s slot %d: parts != single call" % (name, k)
        _wgrad_close(first[k][0].cpu().numpy(), refs[k][0], "%s slot %d dw" % (name, k))
        if dbs[k] is not None:
            _wgrad_close(first[k][1].cpu().numpy(), refs[k][1], "%s slot %d db" % (name, k))


def test_grouped_wgrad_accumulate(hip):
    """kAddTo through the fold and through the direct write (one split): dw = old + ref."""
    import torch
    from mxdetection_amd.ops import dense
    refs = _wgg_data()["refs"]
    for tune in ({}, R.ONE_SPLIT):
        calls, dws, dbs = _wgg_calls(acc=True)
        old = {}
        for k in dws:
            dws[k].copy_(torch.randn(dws[k].shape, generator=torch.Generator().manual_seed(k)))
            if dbs[k] is not None:
                dbs[k].copy_(torch.randn(dbs[k].shape, generator=torch.Generator().manual_seed(50 + k)))
            old[k] = (dws[k].cpu().double().numpy(), None if dbs[k] is None else dbs[k].cpu().double().numpy())
        with R.steer(tune):
            plan = dense.GroupedWgrad(calls, "cuda")
            ws = torch.full((max(plan.workspace_bytes, 256),), 0xFF, dtype=torch.uint8, device="cuda")
            plan.launch(ws)
            torch.cuda.synchronize()
        for k in dws:
            _wgrad_close(dws[k].cpu().double().numpy() - old[k][0], refs[k][0], "accumulate slot %d dw" % k)
            if dbs[k] is not None:
                _wgrad_close(dbs[k].cpu().double().numpy() - old[k][1], refs[k][1], "accumulate slot %d db" % k)


def test_steering_is_restored(hip):
    for k, i in hip.TUNING_KEYS.items():
        now = hip.load().mxdet_debug_get_tuning(i)
        hip.load().mxdet_debug_set_tuning(i, -1)
        assert hip.load().mxdet_debug_get_tuning(i) == now, k
    plain = dict(kind="fwd", N=2, H=14, W=22, Cin=256, Cout=256, KH=3, KW=3, s=1, p=1, tune={}, force=0)
    assert [R.route_name(r) for r in R.conv_records(plain)] == [R.S64 + " fwd T9"]
