"""Parameter arenas and the convolution layer used by every model part.

Design (MI355X-first, not MXNet's per-NDArray executor):
  * all trainable parameters live in ONE flat fp32 arena (master weights), with a parallel flat fp32
    gradient arena, momentum arena and bf16 working copy. The optimizer is one launch over the arena and
    data-parallel all-reduce works on contiguous slices of the gradient arena (buckets) - no per-tensor
    push/pull as in MXNet's kvstore (/root/reference/README.md:37).
  * parameters are registered in *backward completion order* (box head first, C3 last), so a bucket is a
    contiguous arena slice that becomes final while backward is still running.
  * frozen BatchNorm (use_global_stats) is folded into the filters and a per-channel bias once at
    construction; frozen layers (stem, C2) keep bf16 filters only.
"""
import contextlib
import functools
import math
import os

import torch

from ...ops import dense


def cached_buf(bufs, key, shape, dtype=torch.bfloat16, device=None, zero=False):
    """Activation / gradient buffer cache of a model part, keyed by (name, shape, dtype): a call at another shape
    (inference with 1000 rois per image after training with 512) gets buffers of its own and never frees the ones a
    captured hipGraph holds by address. A head's `_buf` is this function bound to its `bufs` and device (buf_cache)."""
    k = (key, tuple(shape), dtype)
    b = bufs.get(k)
    if b is None:
        b = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=device)
        bufs[k] = b
    return b


def buf_cache(device):
    """(bufs, _buf) of a model part: _buf(key, shape, dtype=bf16, zero=False) is cached_buf on `bufs`."""
    bufs = {}
    return bufs, functools.partial(cached_buf, bufs, device=device)


class Workspace:
    """One caller-owned scratch buffer shared by every wgrad call (the C-ABI never allocates).

    `side` (optional HIP stream): weight-gradient kernels only feed the optimizer, so they are issued on a second
    stream that forks from the main stream at each call (after the producer of dy) and is joined before the
    gradient exchange / optimizer. They then overlap the dgrad chain instead of sitting on its critical path."""
    abl_skip = frozenset()            # detector.py puts the parsed MXDET_ABL_SKIP set here

    def __init__(self, device):
        self.device = device
        self.need = 0
        self.buf = None
        self._retired = []
        self.side = None
        # grouped mode: backward_weight() calls are recorded and issued together at flush() (one launch pair per
        # group -- a ResNet stage, the FPN, a head -- instead of two launches per layer)
        self.grouping = False
        self.pending = []
        self.plans = {}
        self.gbuf = None

    def defer(self, layer, x, dy):
        self.pending.append((layer, x, dy))

    def flush(self):
        """Issue the recorded weight gradients (on the side stream if there is one)."""
        if not self.pending:
            return
        items, self.pending = self.pending, []
        if "wgrad" in self.abl_skip:       # timing-only ablation
            return
        key = tuple((id(l), x.data_ptr(), dy.data_ptr()) for l, x, dy in items)
        plan = self.plans.get(key)
        capturing = torch.cuda.is_current_stream_capturing()
        if plan is None and not capturing:
            calls = [(x, dy, l.k, l.k, l.stride, l.pad, l.arena.view(l.wi, "g"),
                      l.arena.view(l.bi, "g") if l.train_bias else None, False) for l, x, dy in items]
            plan = dense.GroupedWgrad(calls, self.device)
            self.plans[key] = plan
            if self.gbuf is None or self.gbuf.numel() < plan.workspace_bytes:
                self._retired.append(self.gbuf)
                self.gbuf = torch.empty((max(plan.workspace_bytes, 256),), dtype=torch.uint8, device=self.device)
        ctx = self.fork()
        with (ctx if ctx is not None else contextlib.nullcontext()):
            if plan is None or self.gbuf is None or self.gbuf.numel() < plan.workspace_bytes:
                # first seen under capture (no eager warm-up): a table cannot be uploaded now -- per-layer launches
                for l, x, dy in items:
                    dense.conv2d_wgrad(x, dy, l.k, l.k, l.stride, l.pad, l.arena.view(l.wi, "g"),
                                       l.arena.view(l.bi, "g") if l.train_bias else None, False, self.get())
            else:
                plan.launch(self.gbuf)
    def fork(self):
        if self.side is None:
            return None
        self.side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.side)

    def join(self):
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)

    def require(self, nbytes):
        self.need = max(self.need, int(nbytes))

    def get(self):
        if self.buf is None or self.buf.numel() < self.need:
            self._retired.append(self.buf)     # a captured step may hold the old one by address: never freed
            self.buf = torch.empty((self.need,), dtype=torch.uint8, device=self.device)
        return self.buf


class ParamArena:
    def __init__(self, device):
        self.device = device
        self.entries = []   # (name, shape, offset, numel)
        self.size = 0
        self.w = self.g = self.m = self.wb = None

    def register(self, name, shape):
        n = 1
        for s in shape:
            n *= s
        off = self.size
        self.entries.append((name, tuple(shape), off, n))
        self.size += (n + 63) // 64 * 64   # keep every tensor 256-B aligned in the fp32 arena
        return len(self.entries) - 1

    def finalize(self):
        dev = self.device
        self.w = torch.zeros((self.size,), dtype=torch.float32, device=dev)
        self.g = torch.zeros((self.size,), dtype=torch.float32, device=dev)
        self.m = torch.zeros((self.size,), dtype=torch.float32, device=dev)
        self.wb = torch.zeros((self.size,), dtype=torch.bfloat16, device=dev)

    def view(self, idx, which):
        _, shape, off, n = self.entries[idx]
        return getattr(self, which)[off:off + n].view(shape)

    def offset_of(self, idx):
        return self.entries[idx][2]

    def refresh_bf16(self):
        dense.f32_to_bf16(self.w, self.wb)

    def sgd_step(self, lr, momentum, wd, rescale):
        dense.sgd_momentum_update(self.w, self.g, self.m, self.wb, lr, momentum, wd, rescale)


class ConvLayer:
    """conv / fc with fused bias (+residual)(+ReLU); trainable or frozen.

    Filters are [Cout,KH,KW,Cin] bf16; a fully connected layer is KH=KW=1 on [R,1,1,Cin] tensors.
    """

    def __init__(self, name, cin, cout, k, stride=1, pad=None, bias=True, trainable=True, arena=None, ws=None,
                 device="cuda", gen=None, init_std=None, zero_init=False, train_bias=True, cout_real=None):
        self.name, self.cin, self.cout, self.k, self.stride = name, cin, cout, k, stride
        self.pad = (k // 2) if pad is None else pad
        self.trainable = trainable
        self.arena, self.ws = arena, ws
        self.has_bias = bias
        std = init_std if init_std is not None else math.sqrt(2.0 / (k * k * cin))   # He-normal
        w0 = torch.zeros((cout, k, k, cin)) if zero_init else torch.randn((cout, k, k, cin), generator=gen) * std
        # output channels past cout_real are alignment padding (fused / padded head outputs): zero filters and zero
        # biases, and every loss kernel writes zero gradients there, so they stay exactly zero through training
        self.cout_real = cout if cout_real is None else cout_real
        if self.cout_real < cout:
            w0[self.cout_real:] = 0
        self._w0 = w0
        self.train_bias = bias and trainable and train_bias
        self.frozen_bias = None
        if bias and not self.train_bias:   # folded frozen-BN shift: a constant
            self.frozen_bias = torch.zeros((cout,), dtype=torch.float32, device=device)
        if trainable:
            self.wi = arena.register(name + ".weight", (cout, k, k, cin))
            self.bi = arena.register(name + ".bias", (cout,)) if self.train_bias else None
        else:
            self.w_bf16 = w0.to(torch.bfloat16).to(device)
            self.bias_f32 = self.frozen_bias
        self.wt = None
        self.device = device
        # filters to warm while this layer's forward / data gradient runs (the layer executed next); see
        # mxdet_conv_desc_t.prefetch and ResNet.wire_prefetch
        self.pf_fwd = self.pf_bwd = None

    # called after arena.finalize()
    def materialize(self):
        if not self.trainable:
            return
        self.arena.view(self.wi, "w").copy_(self._w0.to(self.device))
        self.w_bf16 = self.arena.view(self.wi, "wb")
        self.bias_f32 = self.arena.view(self.bi, "w") if self.train_bias else self.frozen_bias
        self.wt = torch.empty((self.cin, self.k, self.k, self.cout), dtype=torch.bfloat16, device=self.device)
        self._w0 = None

    def plan(self, x_shape):
        """Reserve wgrad scratch for an input of this shape."""
        if self.trainable:
            self.ws.require(dense.conv2d_wgrad_workspace_bytes(x_shape, self.cout, self.k, self.k, self.stride, self.pad))

    def out_shape(self, x_shape):
        N, H, W, _ = x_shape
        return (N, (H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1,
                self.cout)

    def refresh_transposed(self):
        if self.trainable:
            dense.filter_transpose(self.w_bf16, self.wt)

    def forward(self, x, relu=False, residual=None, res_upsample=False, out=None, bits_out=None):
        """bits_out: uint8 [N,Ho,Wo,Cout/8] receiving the 1-bit ReLU mask of the output (for the backward pass)."""
        if dense.PF_TRACE is not None:
            dense.PF_TRACE.append((self, "f", dense.mem_range(self.w_bf16), None))
        return dense.conv2d_forward(x, self.w_bf16, self.bias_f32, residual, self.stride, self.pad, relu, res_upsample,
                                    out, prefetch=self.pf_fwd, bits_out=bits_out)

    def fwd_call(self, x, relu=False, residual=None, res_upsample=False, out=None, bits_out=None):
        """Argument tuple of this layer's forward for dense.conv2d_group("fwd", ...)."""
        t = (x, self.w_bf16, self.bias_f32, residual, self.stride, self.pad, relu, res_upsample, out)
        return t if bits_out is None else t + (bits_out,)

    def dgrad_call(self, dy, x_shape, residual=None, relu_mask=None, accumulate=False, out=None, relu_bits=None):
        """Argument tuple of this layer's data gradient for dense.conv2d_group("dgrad", ...)."""
        t = (dy, self.wt, tuple(x_shape), self.k, self.k, self.stride, self.pad, residual, relu_mask, accumulate, out)
        return t if relu_bits is None else t + (relu_bits,)

    def backward_data(self, dy, x_shape, residual=None, relu_mask=None, accumulate=False, out=None, relu_bits=None):
        """relu_bits: the 1-bit form of relu_mask (read instead of it: 1/16 of the operand bytes)."""
        if dense.PF_TRACE is not None:
            dense.PF_TRACE.append((self, "b", dense.mem_range(self.wt), None))
        return dense.conv2d_dgrad(dy, self.wt, x_shape, self.k, self.k, self.stride, self.pad, residual,
                                  None if relu_bits is not None else relu_mask, accumulate, out, prefetch=self.pf_bwd,
                                  relu_bits=relu_bits)

    def backward_weight(self, x, dy, accumulate=False):
        if self.ws.grouping and not accumulate:
            self.ws.defer(self, x, dy)
            return
        dw = self.arena.view(self.wi, "g")
        db = self.arena.view(self.bi, "g") if self.train_bias else None
        ctx = self.ws.fork()
        if ctx is None:
            dense.conv2d_wgrad(x, dy, self.k, self.k, self.stride, self.pad, dw, db, accumulate, self.ws.get())
        else:
            with ctx:
                dense.conv2d_wgrad(x, dy, self.k, self.k, self.stride, self.pad, dw, db, accumulate, self.ws.get())


class GroupNormLayer:
    """GroupNorm (+ fused ReLU) after a bias-free convolution of a trainable head (ops/group_norm.py).

    Parameters `<name>.gamma` / `<name>.beta` are fp32 arena entries; the kernels read the master copy (the arena's bf16
    working copy of them is never used), weight decay and the one-launch SGD update treat them like every other entry.
    gamma starts at 1, beta at 0: creating the layer draws no random numbers. It is not a ConvLayer: detectors keep it in
    `norm_layers`, apart from `layers`, so the filter-transpose tables, prefetch wiring and grouped weight-gradient plans
    never see it. backward() writes dgamma / dbeta into the arena's gradient slice on the CURRENT stream; the bucket that
    holds them is closed by DetectorBase._reduce afterwards, whose weight-gradient flush and update fork the side stream
    from the current one (Workspace.fork) -- so the update is ordered behind these writes in eager, grouped and captured
    steps alike (with a gradient exchange the bucket's event node / all-reduce is recorded behind them too)."""
    trainable = True

    def __init__(self, name, channels, groups, arena, device="cuda", eps=1e-5):
        if groups <= 0 or channels % groups or (channels // groups) % 8:
            raise ValueError("GroupNorm %s: %d groups do not divide %d channels into multiples of 8" % (name, groups, channels))
        self.name, self.C, self.G, self.eps = name, channels, groups, eps
        self.arena, self.device = arena, device
        self.gi = arena.register(name + ".gamma", (channels,))
        self.bi = arena.register(name + ".beta", (channels,))
        self.bufs = {}
        self.plans = {}
        self.gamma = self.beta = None
        self.x = self.y = self.mean = self.rstd = None
        self.relu = False

    def materialize(self):
        self.gamma, self.beta = self.arena.view(self.gi, "w"), self.arena.view(self.bi, "w")
        self.gamma.fill_(1.0)
        self.beta.zero_()

    def named_params(self):
        return [(self.name + ".gamma", self.gi), (self.name + ".beta", self.bi)]

    def plan(self, x_shape):
        """Statistics and workspaces for an input of this shape: allocated at the first call for a shape (nothing is
        allocated in a step), looked up afterwards -- forward() / backward() cost one dict lookup, no ABI call."""
        x_shape = tuple(x_shape)
        p = self.plans.get(x_shape)
        if p is None:
            from ...ops import group_norm as GN
            stats = [cached_buf(self.bufs, k, (x_shape[0], self.G), torch.float32, self.device) for k in ("mean", "rstd")]
            ws = [cached_buf(self.bufs, "ws%d" % b, (max(GN.workspace_bytes(x_shape, self.G, bool(b)), 256),), torch.uint8,
                             self.device) for b in (0, 1)]
            p = self.plans[x_shape] = (stats[0], stats[1], ws[0], ws[1])
        return p

    def forward(self, x, relu=False, out=None):
        from ...ops import group_norm as GN
        mean, rstd, ws, _ = self.plan(x.shape)
        y, _, _ = GN.group_norm_forward(x, self.gamma, self.beta, self.G, self.eps, relu, out=out, mean=mean, rstd=rstd,
                                        workspace=ws)
        self.x, self.y, self.mean, self.rstd, self.relu = x, y, mean, rstd, relu
        return y

    def backward(self, dy, out=None):
        """dx; dgamma / dbeta go to the arena's gradient slice. The ReLU mask is recomputed from x (a third fewer bytes
        than reading y; the same bits: tests/test_gpu_group_norm.py)."""
        from ...ops import group_norm as GN
        return GN.group_norm_backward(self.x, dy, self.mean, self.rstd, self.gamma, self.G, self.arena.view(self.gi, "g"),
                                      self.arena.view(self.bi, "g"), y=None, beta=self.beta, eps=self.eps, relu=self.relu,
                                      out=out, workspace=self.plan(self.x.shape)[3])


class ContextBlock:
    """The global context block of GCNet (Cao et al. 2019; ops/context.py) between a bottleneck's conv3
    and its shortcut add: attention pooling of t = conv3's output, Linear C -> P = C / reduction, LayerNorm, ReLU, Linear
    P -> C, and y = relu(t + add + shortcut) in one fused pass.

    Seven arena entries, registered in the order their gradients complete: `<name>.fc2.weight` [C,P], `.fc2.bias` [C],
    `.ln.gamma` [P], `.ln.beta` [P], `.fc1.weight` [P,C], `.fc1.bias` [P], `.mask.weight` [C] (the 1x1 attention filter; it has
    no bias: a softmax ignores a shift). The kernels read the three filters from the arena's bf16 working copy and the four
    1-D arrays from the fp32 master. fc2 starts at zero, so a new block computes relu(t + shortcut); the mask filter and fc1 are
    He-normal draws from `gen`, the blocks' own generator; gamma = 1, beta = 0, fc1.bias = 0.
    Like GroupNormLayer it is no ConvLayer: detectors keep it in `norm_layers`, and backward() writes its gradients into the
    arena's gradient slice on the CURRENT stream, before the bucket that holds them is closed (GroupNormLayer's docstring
    gives the ordering argument)."""
    trainable = True
    PARTS = ("fc2.weight", "fc2.bias", "ln.gamma", "ln.beta", "fc1.weight", "fc1.bias", "mask.weight")

    def __init__(self, name, C, reduction, arena, device="cuda", gen=None, eps=1e-5):
        from ...ops import context
        if not isinstance(reduction, int) or isinstance(reduction, bool) or reduction <= 0 or C % reduction:
            raise ValueError("global context block %s: reduction %r does not divide %d channels" % (name, reduction, C))
        P = C // reduction
        context.check_shape(C, P)
        self.name, self.C, self.P, self.eps = name, C, P, eps
        self.arena, self.device = arena, device
        shapes = {"fc2.weight": (C, P), "fc2.bias": (C,), "ln.gamma": (P,), "ln.beta": (P,), "fc1.weight": (P, C),
                  "fc1.bias": (P,), "mask.weight": (C,)}
        self.idx = {p: arena.register("%s.%s" % (name, p), shapes[p]) for p in self.PARTS}
        std = math.sqrt(2.0 / C)
        self._w0 = {"mask.weight": torch.randn((C,), generator=gen) * std, "fc1.weight": torch.randn((P, C), generator=gen) * std}
        self.plans = {}
        self.plan_ = None

    def materialize(self):
        for p, i in self.idx.items():
            w = self.arena.view(i, "w")
            if p in self._w0:
                w.copy_(self._w0[p].to(self.device))
            else:
                w.fill_(1.0 if p == "ln.gamma" else 0.0)
        self._w0 = None

    def named_params(self):
        return [("%s.%s" % (self.name, p), self.idx[p]) for p in self.PARTS]

    def _v(self, part, which):
        return self.arena.view(self.idx[part], which)

    def plan(self, N, HW):
        """The plan (descriptor, statistics, workspace) for maps of N x HW positions: made at the first call for a shape."""
        p = self.plans.get((N, HW))
        if p is None:
            from ...ops.context import ContextPlan
            p = self.plans[(N, HW)] = ContextPlan(N, HW, self.C, self.P, self.device, self.eps)
        return p

    def forward(self, t, sc, out, bits_out=None):
        """out = bf16(relu(t + add + sc)) (and its 1-bit mask); t, sc, out bf16 [N,H,W,C]."""
        p = self.plan_ = self.plan(t.shape[0], t.shape[1] * t.shape[2])
        p.pool_forward(t, self._v("mask.weight", "wb"))
        p.transform_forward(self._v("fc1.weight", "wb"), self._v("fc1.bias", "w"), self._v("ln.gamma", "w"), self._v("ln.beta", "w"),
                            self._v("fc2.weight", "wb"), self._v("fc2.bias", "w"))
        return p.fuse_forward(t, sc, out, bits_out)

    def backward(self, t, ds, d_t):
        """d_t: the gradient w.r.t. t (ds is that of the pre-activation sum, already masked); the seven parameter gradients
        go to the arena's gradient slice."""
        p = self.plan_
        p.reduce_backward(ds)
        p.transform_backward(self._v("fc1.weight", "wb"), self._v("ln.gamma", "w"), self._v("ln.beta", "w"),
                             self._v("fc2.weight", "wb"), self._v("fc1.weight", "g"), self._v("fc1.bias", "g"),
                             self._v("ln.gamma", "g"), self._v("ln.beta", "g"), self._v("fc2.weight", "g"), self._v("fc2.bias", "g"))
        return p.pool_backward(t, self._v("mask.weight", "wb"), ds, d_t, self._v("mask.weight", "g"))


def fc_ksplit():
    """MXDET_TUNE_FC1_KSPLIT (read when a head is built, never in a step): the split of fc_forward, 1 = never split."""
    return int(os.environ.get("MXDET_TUNE_FC1_KSPLIT", "4"))


def fc_forward(fc, x, ksplit, buf, relu=True, out=None):
    """Forward of an FC (1x1 ConvLayer on [R,1,1,C]) whose reduction may be split `ksplit` ways.

    The fc1 of a box head is 196 K-steps on 16 x 16 tiles of 64 x 64: one latency-bound wave per SIMD on its own (118 us
    in the step while nothing else runs). Split four ways the grid fills the chip; the fold is deterministic (split
    order). The split kernel takes whole 64-row tiles only; every other shape runs the plain kernel."""
    R = x.shape[0]
    if ksplit > 1 and (R * fc.cout) % (64 * 64 * 8) == 0 and R % 64 == 0:
        ws = buf(("splitk", fc.name), (4 * ksplit * R * fc.cout,), dtype=torch.uint8)
        return dense.conv2d_forward_splitk(x, fc.w_bf16, fc.bias_f32, None, relu, ksplit, out, ws)
    return fc.forward(x, relu=relu, out=out)


class LayerChain:
    """A sequence of ConvLayers, each followed by an optional GroupNorm and an optional ReLU: the conv towers and FC trunks
    of the RoI heads (an FC is a 1x1 conv on [R,1,1,C]; the `view` between a tower and an FC stays with the head).

    `specs`: one dict per layer in forward order -- ConvLayer's name, cin, cout, k and optionally stride, init_std,
    cout_real, zero_init, plus two keys of the chain: `relu` (default True) and `split` (default False: True sends the
    layer's forward through fc_forward). norm = "gn": every conv is bias-free and followed by GroupNorm `<name>_gn`, into
    whose kernel the ReLU is fused.

    The chain fixes the two orders that nothing downstream can check:
      * registration = backward completion order: for i descending, GN i, then conv i -- so are the generator's draws;
      * backward, per layer from last to first: GN backward, weight gradient, data gradient. The data gradient of layer
        i applies the ReLU that produced its input acts[i], i.e. layer i-1's; with GN none does (the GN backward applies its
        own); layer 0's input belongs to the caller, who names its mask (`first_mask`), as `out_mask` names this chain's
        for whoever computes the gradient of its output.
    Buffers come from the owner's `_buf`, keyed by layer name."""

    def __init__(self, specs, arena, ws, device, gen, norm="none", gn_groups=32):
        n = len(specs)
        self.gn = norm == "gn"
        self.relu = [s.get("relu", True) for s in specs]
        self.split = [s.get("split", False) for s in specs]
        self.ksplit = fc_ksplit() if any(self.split) else 1
        self.convs, self.norms = [None] * n, [None] * n
        for i in reversed(range(n)):
            s = {k: v for k, v in specs[i].items() if k not in ("relu", "split")}
            if self.gn:
                self.norms[i] = GroupNormLayer(s["name"] + "_gn", s["cout"], gn_groups, arena, device)
            self.convs[i] = ConvLayer(bias=not self.gn, arena=arena, ws=ws, device=device, gen=gen, **s)
        self.acts = None

    def layers(self):
        return list(reversed(self.convs))

    def norm_layers(self):
        return [n for n in reversed(self.norms) if n is not None]

    def plan(self, x_shape):
        for c, n in zip(self.convs, self.norms):
            c.plan(x_shape)
            x_shape = c.out_shape(x_shape)
            if n is not None:
                n.plan(x_shape)
        return x_shape

    def forward(self, x, buf):
        """Keeps acts = [x, output of layer 0, ...]; returns the last."""
        self.acts = [x]
        for c, n, relu, split in zip(self.convs, self.norms, self.relu, self.split):
            out = buf(("a", c.name), c.out_shape(x.shape))
            if n is not None:
                x = n.forward(c.forward(x, out=buf(("c", c.name), out.shape)), relu=relu, out=out)
            elif split:
                x = fc_forward(c, x, self.ksplit, buf, relu=relu, out=out)
            else:
                x = c.forward(x, relu=relu, out=out)
            self.acts.append(x)
        return x

    def _mask(self, i):
        return self.acts[i] if i > 0 and self.relu[i - 1] and not self.gn else None

    @property
    def out_mask(self):
        """The ReLU mask that the data gradient arriving at this chain's output has to apply (None: no ReLU there, or GN's
        backward applies it)."""
        return self._mask(len(self.convs))

    def backward(self, g, buf, first_mask=None, add_to=None):
        """g: the gradient of the output, already masked by out_mask. Returns the gradient of the input -- added into
        `add_to` if given (a second branch on the same input), else in a buffer of the chain's."""
        for i in reversed(range(len(self.convs))):
            c, n, x = self.convs[i], self.norms[i], self.acts[i]
            if n is not None:
                g = n.backward(g, out=buf(("dn", c.name), g.shape))
            c.backward_weight(x, g)
            mask = self._mask(i) if i > 0 else first_mask
            if i == 0 and add_to is not None:
                g = c.backward_data(g, x.shape, relu_mask=mask, accumulate=True, out=add_to)
            else:
                g = c.backward_data(g, x.shape, relu_mask=mask, out=buf(("g", c.name), x.shape))
        return g


class DeformConvLayer:
    """3x3 deformable convolution (DCN v1, or v2 with `modulated`), MXNet role contrib.DeformableConvolution; the
    drop-in for a bottleneck's conv2 ("Deformable convolution").

    Two trainable parts:
      * `offset`: a plain 3x3 ConvLayer at the layer's stride, with bias, that predicts the offsets (and v2 mask logits)
        -- 18G (27G) real output channels padded to a multiple of 64 (mxdet_conv2d_dgrad needs Cout % 64), zero at
        the start as DCN prescribes (a zero filter draws no random numbers, so the rest of a model initialises exactly
        as without DCN);
      * `conv`: the deformable filter [Cout,3,3,C] held as the 1x1 filter [Cout,1,1,9C] of the column tensor (same bytes,
        same He-normal draw). Checkpoints store it in OIHW [Cout,C,3,3] under this layer's plain name (dcn_khwc).
    Forward: offset conv -> im2col -> 1x1 forward on col (bias, ReLU, 1-bit mask from the existing epilogue). col is
    kept for the backward pass. Backward: 1x1 data gradient into dcol -> col2im_coord (doff) -> col2im (unmasked dx) ->
    offset-conv data gradient with residual = dx and the input's ReLU mask; the weight gradients of both parts go
    through Workspace.defer like every other layer's."""

    def __init__(self, name, cin, cout, stride=1, groups=1, modulated=True, arena=None, ws=None, device="cuda", gen=None,
                 train_bias=False):
        self.name, self.cin, self.cout, self.stride, self.pad = name, cin, cout, stride, 1
        self.groups, self.modulated = groups, bool(modulated)
        self.k = 3
        self.trainable = True
        self.conv = ConvLayer(name, 9 * cin, cout, 1, 1, 0, arena=arena, ws=ws, device=device, gen=gen,
                              train_bias=train_bias)
        self.conv.dcn_khwc = (3, 3, cin)
        nreal = (27 if self.modulated else 18) * groups
        self.offset = ConvLayer(name + "_offset", cin, (nreal + 63) // 64 * 64, 3, stride, 1, arena=arena, ws=ws,
                                device=device, gen=gen, zero_init=True, cout_real=nreal)
        self.ws = ws
        self.device = device
        self.bufs, self._buf = buf_cache(device)
        self.x = self.off = self.col = None

    def layers(self):
        """Registration (= backward completion) order: the deformable filter's gradient is final first."""
        return [self.conv, self.offset]

    def out_shape(self, x_shape):
        return self.offset.out_shape(x_shape)[:3] + (self.cout,)

    def plan(self, x_shape):
        N, Ho, Wo, _ = self.out_shape(x_shape)
        self.offset.plan(x_shape)
        self.conv.plan((N, Ho, Wo, 9 * self.cin))

    def forward(self, x, relu=False, residual=None, out=None, bits_out=None):
        from ...ops import deform_conv
        N, Ho, Wo, _ = self.out_shape(x.shape)
        off = self.offset.forward(x, out=self._buf("off", (N, Ho, Wo, self.offset.cout)))
        col = deform_conv.im2col(x, off, self.stride, self.pad, self.groups, self.modulated,
                                 out=self._buf("col", (N, Ho, Wo, 9 * self.cin)))
        self.x, self.off, self.col = x, off, col
        return self.conv.forward(col, relu=relu, residual=residual, out=out, bits_out=bits_out)

    def backward_weight(self, x, dy, accumulate=False):
        """The deformable filter's gradient (1x1 on col); the offset conv's follows in backward_data, once doff exists."""
        self.conv.backward_weight(self.col, dy, accumulate)

    def backward_data(self, dy, x_shape, residual=None, relu_mask=None, accumulate=False, out=None, relu_bits=None):
        from ...ops import deform_conv
        assert residual is None and not accumulate, "DeformConvLayer.backward_data: no residual / accumulate"
        x_shape = tuple(x_shape)
        dcol = self.conv.backward_data(dy, self.col.shape, out=self._buf("dcol", self.col.shape))
        a = (self.stride, self.pad, self.groups, self.modulated)
        doff = deform_conv.col2im_coord(self.x, self.off, dcol, *a, out=self._buf("doff", self.off.shape))
        nws = deform_conv.col2im_workspace_bytes(x_shape, *a, self.off.shape[3])
        dxu = deform_conv.col2im(self.off, dcol, x_shape, *a, out=self._buf("dxu", x_shape),
                                 workspace=self._buf("c2i_ws", (max(nws, 256),), torch.uint8))
        self.offset.backward_weight(self.x, doff)
        return self.offset.backward_data(doff, x_shape, residual=dxu, relu_mask=relu_mask, out=out, relu_bits=relu_bits)
