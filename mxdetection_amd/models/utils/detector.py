"""Shared training-step machinery of the detectors: parameter arena bookkeeping, bucketed gradient exchange, hipGraph
capture / replay of the whole step, side-stream weight gradients, optimizer step."""
import contextlib
import os

import torch

from ...utils.hipgraph import GraphEvent
from .checkpoint import CheckpointMixin
from .dp import BucketReducer, make_comm
from .layers import ParamArena, Workspace
from .schedule import CapturedStep, ReplayScratch, ScheduleRecorder, begin_capture, uncovered_ranges


# TIMING-ONLY ablations (tools/ablate_step.sh): MXDET_ABL_SKIP=front,sgd,transpose,wgrad leaves the named component out of the
# replayed step -- results are wrong, only the step time means anything (the marginal cost of a component in the overlapped
# schedule, which the sum of its kernel durations overstates). Never set outside that tool.
_PROBE_STREAMS = []          # candidate streams of DetectorBase._stream_clear_of_the_exchange
_ABL = frozenset(t for t in os.environ.get("MXDET_ABL_SKIP", "").split(",") if t)
Workspace.abl_skip = _ABL


class DetectorBase(CheckpointMixin):
    def _init_base(self, device):
        self.device = device
        self.arena = ParamArena(device)
        self.ws = Workspace(device)
        self.planned = None
        self.dist = None
        self.comm = None
        self.world = 1
        self.captured = None      # CapturedStep, once capture() has run
        self._rec = None          # ScheduleRecorder while capture() runs the step under stream capture
        self._tr_table = None
        self.static_extra = {}
        # Tuning switches: read here, once. MXDET_TUNE_BUCKETS names the reduce points that do NOT close a bucket (see
        # _bucket_here). Single GPU: no exchange to overlap, so everything behind the heads is ONE bucket.
        self._bucket_env = os.environ.get("MXDET_TUNE_BUCKETS")
        self.bucket_merge = "123" if self._bucket_env is None else self._bucket_env
        # Captured step, frozen front end as a graph of its own (capture()): the stem + frozen stages of batch k run on
        # the front stream while step k-1 is still in its weight-gradient tail (they depend on the image only).
        front = os.environ.get("MXDET_TUNE_FRONT_PIPE", "1")
        if front not in ("0", "1"):
            raise ValueError("MXDET_TUNE_FRONT_PIPE must be 0 or 1 (got %r)" % (front,))
        self.front_pipeline = front == "1"
        self.front_probe = os.environ.get("MXDET_TUNE_FRONT_PROBE", "1") == "1"
        self.front_probe_tries = int(os.environ.get("MXDET_TUNE_FRONT_PROBE_TRIES", "4"))
        # filter prefetch hints (_wire_prefetch): 0 none, 1 every launch, 2 not the grouped launches
        self.prefetch = os.environ.get("MXDET_TUNE_PREFETCH", "1")
        self.branch = None
        self._upd = None          # (lr, momentum, wd) while a training step wants its buckets updated as they finish
        self._upd_done = []       # arena ranges already updated in this step
        self._tr_ranges = {}
        self._seen_buckets = set()       # (lo, hi) of every bucket an eager step has exchanged
        self.opt_stream = None

    def _finalize_params(self, layers, frozen_layers=(), norm_layers=()):
        self.layers = layers
        self.norm_layers = list(norm_layers)      # GroupNormLayer: arena parameters without a filter (never transposed)
        self.frozen_layers = list(frozen_layers)
        self.arena.finalize()
        for l in self.layers + self.norm_layers:
            l.materialize()
        self.arena.refresh_bf16()
        self.refresh_transposed()
        self.reducer = BucketReducer(self.arena.g, None)
        # arena offsets after each backbone stage (layer4, layer3, layer2) for bucketed all-reduce
        self.stage_marks = {}
        for si in (3, 2, 1):
            last = self.backbone.stages[si][0].layers()[-1]
            e = self.arena.entries[last.wi]
            self.stage_marks[si] = e[2] + (e[3] + 63) // 64 * 64

    def refresh_transposed(self):
        """[Cout,KH,KW,Cin] -> [Cin,KH,KW,Cout] copies for dgrad: one batched launch for all trainable filters."""
        from ...ops import dense
        if getattr(self, "_tr_table", None) is None:
            pairs = [(l.w_bf16, l.wt) for l in self.layers if l.trainable]
            self._tr_table = dense.make_transpose_table(pairs, self.device)
        dense.filter_transpose_batched(*self._tr_table)

    def enable_wgrad_stream(self):
        """Issue weight-gradient kernels on a second stream (overlaps them with the data-gradient chain)."""
        self.ws.side = torch.cuda.Stream()

    def enable_branch_stream(self):
        """Run the RPN training branch on its own stream, concurrently with the proposal / RoI-head chain."""
        self.branch = torch.cuda.Stream()

    @contextlib.contextmanager
    def _branch_ctx(self):
        """Run the body on the branch stream, concurrently with what the caller issues next on the main stream, until
        _join_branch(). Under capture the body becomes a hipGraph of its own, replayed on the branch stream: two chains
        forked INSIDE one hipGraph did not overlap on this runtime (the second chain's first kernel started about a
        millisecond after the fork, whatever the capture order -- profiles/r01_f_fork_inside_graph.txt), while separate
        graph launches on two streams are at least plain stream semantics. (Measured afterwards: the second chain still
        starts late whenever the first one is running kernels with more workgroups than the chip holds -- the
        dispatcher drains a grid before it serves another queue -- so the gain over the in-graph fork is small; what
        the split did uncover is that memset NODES at the root of a graph do not order against the kernels behind
        them, hence zero_async() in csrc/common.h.)"""
        if self.branch is None:
            yield
            return
        if self._rec is not None:
            with self._rec.branch():
                yield
            return
        self.branch.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.branch):
            yield

    def _join_branch(self):
        if self.branch is None:
            return
        if self._rec is not None:
            self._rec.join_branch()
        else:
            torch.cuda.current_stream().wait_stream(self.branch)

    def enable_data_parallel(self, world_size):
        import torch.distributed as dist
        self.dist = dist
        self.world = world_size
        # RCCL process group: the exchange goes through the library's own collective (mxdet_allreduce_bucket);
        # gloo (CPU tests, two ranks on one GPU): through torch.distributed
        self.comm = make_comm(dist)
        self.reducer = BucketReducer(self.arena.g, dist, comm=self.comm)
        # with a gradient exchange the buckets stay fine (five: every all-reduce but the last overlaps the rest of
        # backward); their weight gradients run as side-stream graphs (_reduce), so fine buckets cost nothing here
        self.bucket_merge = "" if self._bucket_env is None else self._bucket_env

    def broadcast_parameters(self, root=0):
        """Replicate rank `root`'s master weights (and refresh the bf16 / transposed working copies)."""
        if getattr(self, "comm", None) is not None:
            self.comm.broadcast(self.arena.w, root)
        else:
            self.dist.broadcast(self.arena.w, root)
        self.arena.refresh_bf16()
        self.refresh_transposed()

    def _bucket_here(self, point):
        """Reduce points of backward, in order: 0 heads, 1 FPN, 2 layer4, 3 layer3 (layer2 always closes the last
        bucket). A point named in bucket_merge does not close its bucket: the parameters join the next one. Fewer,
        larger buckets mean fewer and better-filled grouped weight-gradient / fold / update launches and fewer
        interruptions of the dgrad chain (whole-step A/B: +1.3…2 % for two buckets instead of five at N = 1)."""
        return str(point) not in self.bucket_merge

    def _guard_replan(self, key):
        """plan() at a new input shape reallocates buffers a captured step holds by address."""
        if (self.captured is not None or self._rec is not None) and self.planned is not None and self.planned != key:
            raise RuntimeError("the captured training step holds the buffers planned for %s; a call at %s would free "
                               "them (build a second model for another input shape)" % (self.planned, key))

    def enable_grouped_wgrad(self):
        """Issue the weight gradients of each bucket (box/mask heads, FPN, every ResNet stage) as one grouped launch."""
        self.ws.grouping = True
        if getattr(self, "ws_rpn", None) is not None:
            self.ws_rpn.grouping = True

    def _reduce(self, lo, hi, pre=None):
        """Close the gradient bucket [lo, hi). pre: another workspace whose recorded weight gradients belong to this
        bucket and go out first, on the same stream (the RPN head's, when they were not issued inside the branch)."""
        rec = self._rec
        exchange = self.dist is not None and hi > lo
        # under capture, with a side stream and grouping: the bucket's weight gradients become a side-stream graph
        # (ScheduleRecorder.close_bucket) instead of being issued here
        on_side = rec is not None and exchange and self.ws.side is not None and self.ws.grouping and bool(self.ws.pending)
        if not on_side:
            if pre is not None:
                pre.side = self.ws.side
                pre.flush()
            self.ws.flush()           # grouped mode: the bucket's recorded weight gradients go out now
            if self.dist is not None:
                # the all-reduce is ordered on the main stream: wait for the side stream's weight gradients. Without an
                # exchange the bucket's update follows its weight gradients ON the side stream and the main stream never
                # waits (optimizer_step / segment ends join the side stream).
                self.ws.join()
        if rec is not None:
            if exchange:
                rec.close_bucket(lo, hi, pre, on_side)
        else:
            self.reducer.reduce(lo, hi)
            if hi > lo:
                self._seen_buckets.add((lo, hi))
        if self._upd is not None and self.dist is None and hi > lo:
            self._update_range(lo, hi)

    def _backbone_backward(self, lo):
        """Backward of backbone stages 4..2 from dC, closing the gradient buckets that begin at arena offset lo."""
        for si in (3, 2, 1):
            self._backbone_stage_backward(si)
            if si == 1:
                self._mark_tail()                          # the data-gradient chain ends here
            if si == 1 or self._bucket_here(5 - si):       # reduce points 2 (layer4), 3 (layer3); layer2 always closes
                self._reduce(lo, self.stage_marks[si])
                lo = self.stage_marks[si]

    def _backbone_stage_backward(self, si):
        stage = self.backbone.stages[si]
        ds = self.dC[si]
        for bi in reversed(range(len(stage))):
            b = stage[bi]
            if bi > 0:
                ds = b.backward(ds, b._buf("dx", b.x.shape), False)
            elif b.need_dx:
                b.backward(ds, self.dC[si - 1], True)
            else:
                b.backward(ds, None, False)

    def _update_range(self, lo, hi):
        """SGD-momentum update + bf16 / transposed working copies of one finished bucket, on the weight-gradient stream:
        nothing issued so far in this step reads these parameters any more, so the update overlaps the rest of the
        backward pass instead of forming a serial tail after it (single-GPU path; with a gradient exchange the update
        follows the last all-reduce, see optimizer_step)."""
        ctx = self.ws.fork()
        with (ctx if ctx is not None else contextlib.nullcontext()):
            self._apply_update(lo, hi, self._upd, 1.0)
        self._upd_done.append((lo, hi))

    def _transpose_table(self, lo, hi):
        from ...ops import dense
        key = (lo, hi)
        if key not in self._tr_ranges:
            a = self.arena
            pairs = [(l.w_bf16, l.wt) for l in self.layers if l.trainable and lo <= a.offset_of(l.wi) < hi]
            self._tr_ranges[key] = dense.make_transpose_table(pairs, self.device) if pairs else None
        return self._tr_ranges[key]

    def _apply_update(self, lo, hi, hyper, rescale):
        """SGD-momentum on arena[lo:hi] + refresh of the bf16 / transposed working copies of that range."""
        from ...ops import dense
        lr, momentum, wd = hyper
        a = self.arena
        if "sgd" not in _ABL:
            dense.sgd_momentum_update(a.w[lo:hi], a.g[lo:hi], a.m[lo:hi], a.wb[lo:hi], lr, momentum, wd, rescale)
        table = self._transpose_table(lo, hi)
        if table is not None and "transpose" not in _ABL:
            dense.filter_transpose_batched(*table)

    # ---- hipGraph capture of the whole step (static shapes): removes ~450 host launches per step ----

    @contextlib.contextmanager
    def _weights_restored(self):
        """Eager steps run in the body plan shapes and allocate buffers only: parameters, momentum, the bf16 /
        transposed working copies and a model's other step state (_step_state) are put back afterwards."""
        snap = (self.arena.w.clone(), self.arena.m.clone(), self._step_state())
        yield
        torch.cuda.synchronize()
        self.arena.w.copy_(snap[0])
        self.arena.m.copy_(snap[1])
        self._set_step_state(snap[2])
        self.arena.refresh_bf16()
        self.refresh_transposed()
        del snap
        torch.cuda.synchronize()

    def _step_state(self):
        """Device state outside the arena that a training step mutates (none here; RetinaNet: the GHM moving average).
        _weights_restored hands what this returns back to _set_step_state."""
        return None

    def _set_step_state(self, state):
        pass

    def capture(self, image, gt_boxes, im_info, lr, image_offset=0, warmup=2, gt_masks=None, momentum=0.9, wd=1e-4,
                gt_keypoints=None):
        """Capture forward+backward+update into hipGraph segments (cut only at gradient all-reduces).
        The RNG step counter is read from device memory (step_dev), inputs from static buffers. momentum / wd are
        baked into the captured update kernels (lr is read from device memory: replay(lr=...)). The eager warm-up
        steps plan shapes and allocate buffers only: parameters and momentum are restored afterwards, so replay(step=0)
        is the first training step, exactly as train_step(step=0) on a fresh model would be."""
        dev = self.device
        hyper = (float(momentum), float(wd))
        self.static_in = (image.clone(), gt_boxes.clone(), im_info.clone())
        self.static_masks = gt_masks.clone() if gt_masks is not None else None
        self.static_keypoints = gt_keypoints.clone() if gt_keypoints is not None else None
        kp = {} if gt_keypoints is None else {"gt_keypoints": self.static_keypoints}     # models without the head take none
        self.step_dev = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=dev)   # replay(lr=...) rewrites it
        self._lr_host = lr

        def eager_step(step):
            self.train_step(*self.static_in, step=step, image_offset=image_offset, lr=lr, gt_masks=self.static_masks,
                            momentum=hyper[0], wd=hyper[1], **kp)
        if warmup > 0:
            with self._weights_restored():
                for i in range(warmup):     # eager warm-up: plans shapes and allocates every buffer
                    eager_step(i)
        torch.cuda.synchronize()
        cap = CapturedStep()
        update_hyper = None       # (lr, momentum, wd) of per-bucket update graphs (N > 1)
        if self.dist is not None and self._seen_buckets:
            # buckets seen in the eager warm-up: their transpose tables are built here, outside any capture
            # The per-bucket updates get no stream of their own when the RPN branch has one: HIP multiplexes streams onto
            # four hardware queues, and a fifth stream shared the main stream's queue -- every update graph (it waits for
            # its bucket's all-reduce) then blocked the data-gradient chain queued behind it (measured at world size 1:
            # 375 vs 422 img/s for the schedule without an exchange). The branch stream is idle by the time the first
            # bucket closes (the branch is joined before the RoI backward) and must wait for the updates anyway before
            # the next step's RPN branch reads the weights.
            self.opt_stream = self.branch if self.branch is not None else torch.cuda.Stream()
            update_hyper = (self.lr_dev,) + hyper
            for lo_hi in sorted(self._seen_buckets):
                self._transpose_table(*lo_hi)
        # exactly one frozen stage: with more, forward_rest has no C2 to hand to the FPN under front_override
        use_front = self.front_pipeline and self.backbone.frozen_front() == 1 and warmup > 0
        if use_front:
            # the second output buffer of the front end and every plan keyed by it (grouped launches of the consumers)
            # must exist before a capture: one more eager step on parity 1
            with self._weights_restored():
                self.backbone.eager_parity = 1
                eager_step(0)
                self.backbone.eager_parity = 0
            cap.tail_event = GraphEvent()
            cap.front_stream = self.branch if self.branch is not None else torch.cuda.Stream()
            if self.dist is not None and getattr(self.reducer, "comm", None) is not None and self.front_probe:
                cap.front_stream = self._stream_clear_of_the_exchange(cap.front_stream)
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        for parity in ((0, 1) if use_front else (0,)):
            front = None
            if use_front:
                # the front end of this parity: its own graph, captured on the front stream
                cap.front_stream.wait_stream(cur)
                front = torch.cuda.CUDAGraph()
                with torch.cuda.stream(cap.front_stream):
                    begin_capture(front, cap.pool_front)
                    c2 = self.backbone.forward_front(self.static_in[0], parity)
                    front.capture_end()
                cur.wait_stream(cap.front_stream)
                self.backbone.front_override = c2
            with torch.cuda.stream(side):
                self._rec = ScheduleRecorder(self, cap, update_hyper)
                self._rec.seg_begin()
                self._upd, self._upd_done = (((self.lr_dev,) + hyper) if self.dist is None else None), []
                losses = self.forward_backward(*self.static_in, step=0, image_offset=image_offset, step_dev=self.step_dev,
                                               gt_masks=self.static_masks, **kp)
                self._upd = None
                self.optimizer_step(self.lr_dev, hyper[0], hyper[1])
                self._rec.finish(front, losses)        # detaches itself
        self.backbone.front_override = None
        cur.wait_stream(side)
        torch.cuda.synchronize()
        if use_front:
            cap.tail_event.record()            # the first replayed step has no predecessor to wait for
            torch.cuda.synchronize()
        self.captured = cap

    def _stream_clear_of_the_exchange(self, preferred):
        """A stream on which work is NOT held up while an all-reduce waits for its bucket's weight gradients.

        HIP multiplexes streams onto a few hardware queues (four), in order of first use, and a stream that waits for an
        event holds up every stream sharing its queue. During the weight-gradient tail of a step the communicator (its own
        stream and RCCL's internal ones) has such a wait pending most of the time; the next step's front end has to run
        beside that tail, so its stream must not share a queue with any of them (measured at world size 1: on the branch
        stream the front end started only after the step's last all-reduce, and the pipeline's gain was lost). Which queue a
        stream got cannot be asked, so it is measured: a long kernel on the weight-gradient stream, ONE all-reduce of a
        scratch tensor behind it (every rank issues the same single collective), a tiny kernel on each candidate; candidates
        whose kernel has finished while the long kernel still runs are clear. Returns `preferred` if it is clear, else the
        first clear candidate, else `preferred`."""
        import time
        comm = self.reducer.comm
        dev = self.arena.g.device
        tries = self.front_probe_tries
        while len(_PROBE_STREAMS) < tries:             # one set per process: every model's probe tries the same streams
            _PROBE_STREAMS.append(torch.cuda.Stream())
        cands = [preferred] + _PROBE_STREAMS[:tries]
        tiny = torch.zeros((64,), device=dev)
        scratch = torch.zeros((64,), device=dev)
        big = torch.empty((1 << 27,), device=dev)                    # 512 MiB: one pass ~0.2 ms
        wstream = self.ws.side if self.ws.side is not None else torch.cuda.Stream()
        for s_ in cands + [wstream]:                                  # first use of every stream: queues are bound now
            with torch.cuda.stream(s_):
                tiny.add_(0.0)
        torch.cuda.synchronize()
        done_long = torch.cuda.Event()
        with torch.cuda.stream(wstream):
            for _ in range(60):                                       # ~10 ms of work in front of the collective
                big.add_(1.0)
            done_long.record()
            ticket = comm.allreduce(scratch)                          # waits behind the long kernels: the pending wait
        evs = []
        for c in cands:
            e = torch.cuda.Event()
            with torch.cuda.stream(c):
                tiny.add_(0.0)
                e.record()
            evs.append(e)
        clear = [False] * len(cands)
        t0 = time.perf_counter()
        while not done_long.query() and time.perf_counter() - t0 < 2.0:
            for i, e in enumerate(evs):
                clear[i] = clear[i] or e.query()
            if all(clear):
                break
        ticket.wait()
        torch.cuda.synchronize()
        del big
        self.front_stream_probe = clear
        for c, ok in zip(cands, clear):
            if ok:
                return c
        return preferred

    def _mark_tail(self):
        """Called by forward_backward where the data-gradient chain has ended and only the last bucket's weight gradients,
        fold and update remain: under capture with the front-end pipeline, an event-record node the NEXT step's front end
        waits for (it then runs beside that tail: HBM-bound frozen convolutions next to MFMA-bound weight gradients)."""
        if self._rec is not None and self._rec.cap.tail_event is not None:
            self._rec.cap.tail_event.record_node()

    def replay(self, image, gt_boxes, im_info, step, gt_masks=None, lr=None, gt_keypoints=None):
        """One training step from the captured graphs; lr (if given) replaces the captured learning rate from here on."""
        si = self.static_in
        cap = self.captured
        if lr is not None and lr != self._lr_host:
            self.lr_dev.fill_(float(lr))
            self._lr_host = lr
        if cap.front_stream is not None:
            # front end of THIS batch on the front stream, behind the previous step's tail mark (not behind its end)
            par = cap.count & 1
            cap.count += 1
            cap.tail_event.wait(cap.front_stream)
            with torch.cuda.stream(cap.front_stream):
                if image is not si[0]:
                    si[0].copy_(image, non_blocking=True)
                if "front" not in _ABL:
                    cap.parities[par].front.replay()
                cap.ready[par].record()
            torch.cuda.current_stream().wait_event(cap.ready[par])
            captured = cap.parities[par]
        else:
            captured = cap.parities[0]
            if image is not si[0]:
                si[0].copy_(image, non_blocking=True)
        if image is not si[0]:
            si[1].copy_(gt_boxes, non_blocking=True)
            si[2].copy_(im_info, non_blocking=True)
            if gt_masks is not None:
                self.static_masks.copy_(gt_masks, non_blocking=True)
            if gt_keypoints is not None:
                self.static_keypoints.copy_(gt_keypoints, non_blocking=True)
        self.step_dev.fill_(step)
        scratch = ReplayScratch()
        for entry in captured.schedule:
            entry.run(self, scratch)
        return captured.losses

    def optimizer_step(self, lr, momentum=0.9, wd=1e-4):
        self.ws.flush()
        self.ws.join()
        done, self._upd_done = self._upd_done, []
        if done:
            # buckets were updated as they finished; update whatever the bucket marks did not cover
            self._upd = (lr, momentum, wd)
            for lo, hi in uncovered_ranges(done, self.arena.size):
                self._update_range(lo, hi)
            self._upd = None
            self.ws.join()
            return
        if self._rec is None:
            self.reducer.wait()
        elif self.dist is not None and self._rec.end_exchange():
            return                               # every bucket has its own update graph
        self.arena.sgd_step(lr, momentum, wd, 1.0 / self.world)
        self.refresh_transposed()

    def train_step(self, image, gt_boxes, im_info, step=0, image_offset=0, lr=0.0025, gt_masks=None,
                   momentum=0.9, wd=1e-4, gt_keypoints=None):
        self._upd, self._upd_done = ((lr, momentum, wd) if self.dist is None else None), []
        from ...ops import dense
        trace = not getattr(self, "_pf_wired", False) and self.prefetch != "0"
        if trace:
            dense.PF_TRACE = []
        try:
            kp = {} if gt_keypoints is None else {"gt_keypoints": gt_keypoints}
            losses = self.forward_backward(image, gt_boxes, im_info, step, image_offset, gt_masks=gt_masks, **kp)
        finally:
            self._upd = None
            if trace:
                self._wire_prefetch(dense.PF_TRACE)
                dense.PF_TRACE = None
        self.optimizer_step(lr, momentum, wd)
        return losses

    def _wire_prefetch(self, trace):
        """Prefetch hints from the issue order of the first eager step: every single convolution launch names the filter
        the NEXT convolution launch (single or grouped, forward or data gradient) reads, so that it is warm in the
        Infinity Cache when that launch starts (mxdet_conv_desc_t.prefetch; +2 % on the step for the backbone chain
        alone). A layer launched more than once per direction (heads shared across pyramid levels) keeps its last
        successor. The order is the host's issue order: launches of the RPN branch interleave as they were issued."""
        from ...ops import dense
        for (layer, kind, w, key), (_, _, nxt, _) in zip(trace[:-1], trace[1:]):
            if nxt is None or nxt == w:          # the same filter again (a head shared across pyramid levels)
                continue
            if kind == "f":
                layer.pf_fwd = nxt
            elif kind == "b":
                layer.pf_bwd = nxt
            elif key is not None and self.prefetch != "2":
                dense.GROUP_HINTS[key] = nxt     # grouped launch: its table is rebuilt with the hint at the next eager call
                dense._group_plans.pop(key, None)
        self._pf_wired = True
