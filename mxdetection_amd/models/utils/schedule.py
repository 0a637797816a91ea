"""The captured training step as data: the entries of a replayed schedule (one class per kind, each with its part of
DetectorBase.replay), the recorder that builds a schedule while DetectorBase.capture() runs the step under stream
capture, and the object capture() leaves behind."""
import collections
import contextlib
import warnings

import torch

from ...utils.hipgraph import GraphEvent


def uncovered_ranges(ranges, size):
    """The parts of [0, size) that none of the (lo, hi) ranges covers, in order."""
    gaps, pos = [], 0
    for lo, hi in sorted(ranges):
        if lo > pos:
            gaps.append((pos, lo))
        pos = max(pos, hi)
    if pos < size:
        gaps.append((pos, size))
    return gaps


# ---- schedule entries: run(m, scratch) is that entry's part of one replayed step, issued from the main stream ----

class ReplayScratch:
    """What the entries of ONE replayed step hand to each other."""
    __slots__ = ("fork_ev", "handles")

    def __init__(self):
        self.fork_ev = None       # recorded by Fork, waited for by Branch
        self.handles = {}         # bucket index -> work handles of its all-reduce (BucketReduce -> BucketUpdate)


class MainGraph:
    """A segment of the step's main stream."""
    __slots__ = ("graph",)

    def __init__(self, graph):
        self.graph = graph

    def run(self, m, scratch):
        self.graph.replay()


class Fork:
    """The point of the main stream the next Branch starts behind."""
    __slots__ = ()

    def run(self, m, scratch):
        scratch.fork_ev = torch.cuda.Event()
        scratch.fork_ev.record()


class Branch:
    """A graph replayed on the branch stream, beside the main segments that follow."""
    __slots__ = ("graph",)

    def __init__(self, graph):
        self.graph = graph

    def run(self, m, scratch):
        m.branch.wait_event(scratch.fork_ev)
        with torch.cuda.stream(m.branch):
            self.graph.replay()


class Join:
    __slots__ = ()

    def run(self, m, scratch):
        torch.cuda.current_stream().wait_stream(m.branch)


class BucketWgrad:
    """A bucket's weight gradients: a graph on the side stream, behind the event node that follows the producers of the
    bucket's dy / x in the main graph. The graph is filled in by the deferred capture."""
    __slots__ = ("event", "graph")

    def __init__(self, event, graph=None):
        self.event, self.graph = event, graph

    def run(self, m, scratch):
        self.event.wait(m.ws.side)
        with torch.cuda.stream(m.ws.side):
            self.graph.replay()


class BucketReduce:
    """All-reduce of bucket k = arena.g[lo:hi]; on_side: issued from the side stream, behind the bucket's weight gradients."""
    __slots__ = ("lo", "hi", "k", "on_side")

    def __init__(self, lo, hi, k, on_side):
        self.lo, self.hi, self.k, self.on_side = lo, hi, k, on_side

    def run(self, m, scratch):
        if self.on_side:
            with torch.cuda.stream(m.ws.side):
                scratch.handles[self.k] = m.reducer.reduce(self.lo, self.hi)
        else:
            scratch.handles[self.k] = m.reducer.reduce(self.lo, self.hi)


class BucketUpdate:
    """Bucket k's update graph on the optimizer stream, behind the bucket's sums."""
    __slots__ = ("k", "graph")

    def __init__(self, k, graph=None):
        self.k, self.graph = k, graph

    def run(self, m, scratch):
        with torch.cuda.stream(m.opt_stream):
            for h in scratch.handles.get(self.k, ()):
                h.wait()                       # orders the optimizer stream after the bucket's sums
            self.graph.replay()


class JoinUpdates:
    """End of a step whose buckets each had their own update graph."""
    __slots__ = ()

    def run(self, m, scratch):
        torch.cuda.current_stream().wait_stream(m.opt_stream)
        if m.ws.side is not None:
            torch.cuda.current_stream().wait_stream(m.ws.side)
        m.reducer.pending, m.reducer.log = [], []


class WaitExchange:
    """Every all-reduce issued so far is waited for on the main stream (one update of the whole arena follows)."""
    __slots__ = ()

    def run(self, m, scratch):
        m.reducer.wait()


# ---- capture ----

def begin_capture(graph, pool):
    # thread_local: HIP calls of other threads (RCCL's watchdog, loader workers) must not invalidate the capture
    graph.capture_begin(pool=pool, capture_error_mode="thread_local")


class ScheduleRecorder:
    """Attached to a model (m._rec) while capture() runs one step under stream capture: the model's step code calls it
    wherever the eager step would fork, join, exchange or update; it cuts the main stream into graphs and notes the
    entries in between. finish() hands the result to the CapturedStep."""

    def __init__(self, m, cap, hyper):
        self.m, self.cap = m, cap
        self.hyper = hyper            # (lr_dev, momentum, wd) of the per-bucket update graphs; None: no such graphs
        self.graph = None             # the open main segment
        self.entries = []
        self.markers = []             # bucket entries recorded inside the open segment: they follow its launch
        self.deferred = []            # (entry, stash): bucket graphs still to be captured (finish)
        self.buckets = []             # (lo, hi) of every bucket exchanged in the step
        self.join_updates = False

    def seg_begin(self):
        self.graph = torch.cuda.CUDAGraph()
        begin_capture(self.graph, self.cap.pool_main)

    def seg_end(self):
        """Close the open segment. A segment in which nothing was launched (the step opens with a fork to the branch
        stream) is dropped instead of being replayed as an empty graph every step; torch reports that case with a
        warning at capture_end, which is the only place the node count is visible from Python."""
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            self.graph.capture_end()
        empty = False
        for w in rec:
            if "Graph is empty" in str(w.message):
                empty = True
            else:
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
        if not empty:
            self.entries.append(MainGraph(self.graph))
            self.entries.extend(self.markers)
            self.markers = []
        else:
            assert not self.markers, "bucket markers in an empty graph segment"
            # kept alive, never replayed: destroying the only graph of a memory pool releases the pool, and the next
            # capture_begin on it trips an allocator assertion
            self.cap.empty_graphs.append(self.graph)
        self.graph = None

    def join_branch(self):
        self.m.ws.join()              # a segment cannot end with weight-gradient work still forked
        self.seg_end()
        self.entries.append(Join())
        self.seg_begin()

    @contextlib.contextmanager
    def branch(self):
        """The body becomes a graph of its own on the branch stream (see DetectorBase._branch_ctx)."""
        m = self.m
        cur = torch.cuda.current_stream()
        m.ws.join()
        self.seg_end()
        self.entries.append(Fork())
        g = torch.cuda.CUDAGraph()
        m.branch.wait_stream(cur)
        with torch.cuda.stream(m.branch):
            begin_capture(g, self.cap.pool_branch)
            yield
            g.capture_end()
        cur.wait_stream(m.branch)
        self.entries.append(Branch(g))
        self.seg_begin()

    def close_bucket(self, lo, hi, pre, on_side):
        """The exchange of bucket [lo, hi) and what hangs on it (DetectorBase._reduce under capture)."""
        m = self.m
        k = len(self.buckets)
        self.buckets.append((lo, hi))
        if on_side:
            # No cut of the main graph: an event-record NODE marks the point where this bucket's dy / x exist, and the
            # bucket's weight gradients (a graph of their own, replayed on the side stream behind that event), its
            # all-reduce (issued from the side stream, behind them) and its update (a graph on the optimizer stream,
            # behind the all-reduce's ticket) never touch the main stream. The two small graphs are captured after
            # the main capture (capture_deferred): the recorded weight-gradient calls are stashed here. (Before, the
            # main stream was cut into a segment per bucket and every cut was a 14-32 us hole: -2.9 % at world 1.)
            ev = GraphEvent()
            ev.record_node()
            wgrad = BucketWgrad(ev)
            items_pre = []
            if pre is not None:
                items_pre, pre.pending = pre.pending, []
            items, m.ws.pending = m.ws.pending, []
            self.deferred.append((wgrad, (pre, items_pre, items)))
            self.markers += [wgrad, BucketReduce(lo, hi, k, True)]
            if self.hyper is not None:
                update = BucketUpdate(k)
                self.deferred.append((update, None))
                self.markers.append(update)
            return
        # no side-stream graph: cut the main graph here, the all-reduce runs between segments
        self.seg_end()
        self.entries.append(BucketReduce(lo, hi, k, False))
        if self.hyper is not None:
            # The bucket's update is a small graph of its own, replayed on the optimizer stream once that
            # stream has waited for the bucket's all-reduce: it overlaps the rest of backward exactly like
            # the single-GPU path, and the main stream never waits for a collective before the end of the step.
            cur = torch.cuda.current_stream()
            m.opt_stream.wait_stream(cur)
            g = self.capture_update_graph(lo, hi)
            cur.wait_stream(m.opt_stream)
            self.entries.append(BucketUpdate(k, g))
        self.seg_begin()

    def capture_update_graph(self, lo, hi):
        m = self.m
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(m.opt_stream):
            begin_capture(g, self.cap.pool_opt)
            m._apply_update(lo, hi, self.hyper, 1.0 / m.world)
            g.capture_end()
        return g

    def end_exchange(self):
        """The update behind a step's exchange (DetectorBase.optimizer_step under capture). -> True: every bucket has its
        own update graph and the step ends by joining them; False: every all-reduce is waited for here, between two
        segments, and the caller updates the whole arena."""
        if self.hyper is not None:
            gaps = uncovered_ranges(self.buckets, self.m.arena.size)
            assert not gaps, "parameter range [%d, %d) belongs to no gradient bucket" % gaps[0]
            self.join_updates = True
            return True
        self.seg_end()
        self.entries.append(WaitExchange())
        self.seg_begin()
        return False

    def finish(self, front, losses):
        """End of the step: close the last segment, detach from the model, then capture the per-bucket weight-gradient
        and update graphs of the exchange schedule (their places in the schedule are the event nodes / entries
        close_bucket left in it)."""
        m = self.m
        self.seg_end()
        if self.join_updates:
            self.entries.append(JoinUpdates())
        m._rec = None
        for entry, stash in self.deferred:
            if stash is None:
                entry.graph = self.capture_update_graph(*self.buckets[entry.k])
                continue
            pre, items_pre, items = stash
            g = torch.cuda.CUDAGraph()
            side, m.ws.side = m.ws.side, None
            with torch.cuda.stream(side):
                begin_capture(g, self.cap.pool_wgrad)
                if pre is not None:
                    pre.side = None
                    pre.pending = items_pre
                    pre.flush()
                m.ws.pending = items
                m.ws.flush()
                g.capture_end()
            m.ws.side = side
            entry.graph = g
        self.cap.parities.append(Parity(front, self.entries, losses))
        self.cap.buckets = self.buckets


# one captured step: the front-end graph (None without the front-end pipeline), the schedule behind it, the losses it writes
Parity = collections.namedtuple("Parity", "front schedule losses")


class CapturedStep:
    """What capture() leaves on the model (m.captured). With the front-end pipeline there are two parities, replayed in
    turn (the front end of batch k writes buffer k & 1); without it, one."""
    __slots__ = ("parities", "front_stream", "ready", "count", "tail_event", "buckets", "empty_graphs",
                 "pool_main", "pool_branch", "pool_opt", "pool_wgrad", "pool_front")

    def __init__(self):
        self.parities = []
        self.front_stream = None      # None: no front-end pipeline
        self.ready = (torch.cuda.Event(), torch.cuda.Event())     # per parity: its front graph has been issued
        self.count = 0                # replays so far
        self.tail_event = None        # recorded by a node of the main graph where the weight-gradient tail begins
        self.buckets = []             # (lo, hi) of every bucket exchanged in the captured step
        self.empty_graphs = []
        # memory pools: graphs that run concurrently must not share (time-multiplexed) temporaries, so the main segments,
        # the branch graphs, the update graphs, the weight-gradient graphs and the front graphs each have one
        self.pool_main, self.pool_branch, self.pool_opt, self.pool_wgrad, self.pool_front = (
            torch.cuda.graph_pool_handle() for _ in range(5))
