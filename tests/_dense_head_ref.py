"""fp64 reference of the dense heads -- a tower of shared conv layers applied to every pyramid level -- forward and an explicit,
hand-written backward: RetinaHead (models/rpn_heads/retina_head.py) and the dense path of RPNHead (models/rpn_heads/rpn_head.py),
for tests/test_gpu_retina_head.py, tests/test_gpu_rpn_head_dense.py and tests/test_gpu_retinanet_parity.py. Built on the single
convolutions of tests/_backbone_ref.py and under its conventions: torch-CPU float64 throughout, maps NHWC, filters
[Cout, KH, KW, Cin] (the padded output channels included: zero filter rows, zero biases), bf16 tensors are float64 tensors that
hold bf16 values, p maps the layers' names ("retina.cls0.weight", "rpn.out.bias", ...) to tensors.

emulate=True rounds to bf16 every map the device stores, in the device's order -- each tower activation, the outputs, each
stored data-gradient map, and a gradient that is added into a stored map once more, as the sum -- and nothing else: weight and
bias gradients stay unrounded sums over the levels (fp32 on the device). The emulated variants exist to MEASURE the error
inherent in the number formats, E = max |emulated - exact| (_backbone_ref.check_rows); no device result enters E.

The backward functions take the ReLU masks as arguments (float64 0/1 maps); the GPU tests pass those of the device's own stored
activations, tests/test_dense_head_ref_cpu.py those of the reference's own forward (_backbone_ref's docstring says why)."""
import torch

from _backbone_ref import F64, _st, conv, conv_dgrad, conv_wgrad


def _bias_grad(dy):
    return dy.sum(dim=(0, 1, 2))


def _add(g, key, t):
    g[key] = t if key not in g else g[key] + t


# ---- RetinaHead -------------------------------------------------------------------------------------------------------------
def retina_head_forward(P, p, num_convs, emulate=False):
    """Per level l: class tower cact[l] = [P_l, a_1, ..., a_n] with a_{i+1} = ReLU(conv3x3(a_i, retina.cls<i>)), the same for the
    box tower (bact, retina.box<i>), co[l] = conv3x3(cact[l][n], retina.cls_out), bo[l] = conv3x3(bact[l][n], retina.box_out):
    no ReLU, every channel of the padded layers. The eight tower filters and the two output filters are shared by all levels."""
    st = _st(emulate)
    cact, bact, co, bo = [], [], [], []
    for x in P:
        for tower, acts in (("cls", cact), ("box", bact)):
            a = [x]
            for i in range(num_convs):
                a.append(st(torch.relu(conv(a[-1], p["retina.%s%d.weight" % (tower, i)], p["retina.%s%d.bias" % (tower, i)]))))
            acts.append(a)
        co.append(st(conv(cact[-1][-1], p["retina.cls_out.weight"], p["retina.cls_out.bias"])))
        bo.append(st(conv(bact[-1][-1], p["retina.box_out.weight"], p["retina.box_out.bias"])))
    return dict(cact=cact, bact=bact, co=co, bo=bo)


def retina_head_masks(fwd):
    """The masks of a forward's own activations: {"cls": [[None, a_1 > 0, ..., a_n > 0] per level], "box": ...}."""
    return {k: [[None] + [(a > 0).to(F64) for a in acts[1:]] for acts in fwd[src]]
            for k, src in (("cls", "cact"), ("box", "bact"))}


def retina_head_backward(P, fwd, p, gco, gbo, masks, emulate=False):
    """RetinaHead.backward. gco / gbo: the gradients w.r.t. co / bo (zero in the padded channels). Stored maps, in the device's
    order: each tower's data gradient after every layer, masked by the activation it arrives at; layer 0 of the class tower
    writes dP[l] (no mask: P belongs to the neck), then layer 0 of the box tower adds into the same stored map -- one more
    rounding when emulating. Returns dP per level, the weight and bias gradients of all ten layers summed over the levels, and
    the towers' stored gradients (dact[tower][l][i], the gradient w.r.t. activation i)."""
    st = _st(emulate)
    n = len(fwd["cact"][0]) - 1
    g, dP, dact = {}, [], {"cls": [], "box": []}
    for l in range(len(P)):
        parts = []
        for tower, acts, dy in (("cls", fwd["cact"][l], gco[l]), ("box", fwd["bact"][l], gbo[l])):
            name = "retina.%s_out" % tower
            _add(g, name + ".weight", conv_wgrad(acts[n], dy, p[name + ".weight"]))
            _add(g, name + ".bias", _bias_grad(dy))
            d = st(masks[tower][l][n] * conv_dgrad(dy, p[name + ".weight"], acts[n].shape))
            stored = {n: d}
            for i in reversed(range(n)):
                name = "retina.%s%d" % (tower, i)
                _add(g, name + ".weight", conv_wgrad(acts[i], d, p[name + ".weight"]))
                _add(g, name + ".bias", _bias_grad(d))
                d = conv_dgrad(d, p[name + ".weight"], acts[i].shape)
                if i > 0:
                    d = st(masks[tower][l][i] * d)
                    stored[i] = d
            parts.append(d)
            dact[tower].append(stored)
        dP.append(st(st(parts[0]) + parts[1]))
    return dict(dP=dP, grads=g, dact=dact)


# ---- RPNHead, dense path ----------------------------------------------------------------------------------------------------
def rpn_head_forward(P, p, emulate=False):
    """t[l] = ReLU(conv3x3(P_l, rpn.conv)), h[l] = conv1x1(t[l], rpn.out), every channel of the padded output layer."""
    st = _st(emulate)
    t = [st(torch.relu(conv(x, p["rpn.conv.weight"], p["rpn.conv.bias"]))) for x in P]
    h = [st(conv(x, p["rpn.out.weight"], p["rpn.out.bias"])) for x in t]
    return dict(t=t, h=h)


def rpn_head_backward(P, fwd, p, gh, masks, dP_prefill, dP_has_grad, emulate=False):
    """RPNHead.backward, dense kernels. gh: the gradient w.r.t. h (zero in the padded channels); masks[l] = (t[l] > 0). The
    stored dt[l] = masks[l] * rpn.out's data gradient; rpn.conv's data gradient overwrites dP[l], or, where dP_has_grad[l], is
    added to what the map held (dP_prefill[l]) and the sum is stored. Returns dP and dt per level and the four parameter
    gradients summed over the levels."""
    st = _st(emulate)
    g, dP, dt = {}, [], []
    for l in range(len(P)):
        t = fwd["t"][l]
        _add(g, "rpn.out.weight", conv_wgrad(t, gh[l], p["rpn.out.weight"]))
        _add(g, "rpn.out.bias", _bias_grad(gh[l]))
        d = st(masks[l] * conv_dgrad(gh[l], p["rpn.out.weight"], t.shape))
        _add(g, "rpn.conv.weight", conv_wgrad(P[l], d, p["rpn.conv.weight"]))
        _add(g, "rpn.conv.bias", _bias_grad(d))
        dx = conv_dgrad(d, p["rpn.conv.weight"], P[l].shape)
        dP.append(st(dP_prefill[l] + dx if dP_has_grad[l] else dx))
        dt.append(d)
    return dict(dP=dP, dt=dt, grads=g)
