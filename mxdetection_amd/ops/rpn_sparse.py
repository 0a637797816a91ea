"""Sparse backward of the RPN head over the HIP C-ABI (include/mxdet.h, mxdet_rpn_sparse_t): the active-cell list of a
step's anchor labels, and the head's data / weight gradients over the listed cells only."""
import ctypes as C

import torch

from .. import _lib
from .._lib import RpnOrderedItemT, RpnSparseT, check, ptr, stream_ptr
from . import dense

ZERO, DT, WGRAD, DGRAD, DTMAP, WGRAD_ORDERED = 1, 2, 4, 8, 16, 32
ALL = ZERO | DT | WGRAD | DGRAD
MAX_SLOTS = 8192


class RPNSparse:
    """Buffers of one pyramid geometry: level_shapes [(H, W)], N images, A anchors per cell, C channels, Ch head channels,
    smax slots. Everything is allocated here; list() and backward() only launch."""

    def __init__(self, level_shapes, N, A, C_, Ch, smax, device):
        self.level_shapes, self.N, self.A, self.C, self.Ch, self.smax = list(level_shapes), N, A, C_, Ch, smax
        self.CT = sum(h * w for h, w in level_shapes)
        i32 = dict(dtype=torch.int32, device=device)
        self.list = torch.full((2 * smax,), -1, **i32)
        self.state = torch.zeros((2,), **i32)
        self.map = torch.full((N * self.CT,), -1, **i32)
        self.dts = torch.zeros((smax, C_), dtype=torch.bfloat16, device=device)
        self.ghs = torch.zeros((smax, Ch), dtype=torch.bfloat16, device=device)
        self._descs = {}
        self.ordered = None       # plan_ordered(): the dense split-K schedule of the head's weight gradients
        self.ordered_work = None

    def plan_ordered(self, calls):
        """calls: the head's 2 L weight-gradient calls as dense.GroupedWgrad takes them (rpn.out's levels, then rpn.conv's).
        Plans them as the dense grouped launch would and keeps that plan's split parameters for WGRAD_ORDERED."""
        L = len(self.level_shapes)
        assert len(calls) == 2 * L
        # (planned once, like the dense plans of Workspace.flush: both keep the tunings of their first eager call, so the
        # two paths stay consistent if a tuning is changed afterwards)
        host = dense.plan_wgrad_group(calls)[0]
        sched = (RpnOrderedItemT * (2 * L))()
        check(_lib.load().mxdet_rpn_ordered_schedule(host, 2 * L, L, sched), "rpn_ordered_schedule")
        self.ordered = sched
        self.ordered_work = torch.zeros((10 * self.smax + 32,), dtype=torch.int32, device=self.list.device)
        self._descs = {}

    def _desc(self, P=None, t=None, tbits=None, gh=None, dP=None, accumulate=None, dt=None):
        L = len(self.level_shapes)
        ops = (P, t, tbits, gh, dP, dt)
        key = tuple(None if o is None else tuple(0 if x is None else x.data_ptr() for x in o) for o in ops)
        key += (None if accumulate is None else tuple(bool(a) for a in accumulate),)
        d = self._descs.get(key)
        if d is None:
            d = RpnSparseT()
            d.num_levels, d.N, d.A, d.C, d.Ch, d.smax = L, self.N, self.A, self.C, self.Ch, self.smax
            for l, (h, w) in enumerate(self.level_shapes):
                d.H[l], d.W[l] = h, w
                d.accumulate[l] = int(bool(accumulate[l])) if accumulate is not None else 0
                for name, o in zip(("P", "t", "tbits", "gh", "dP", "dt"), ops):
                    if o is not None and o[l] is not None:
                        getattr(d, name)[l] = o[l].data_ptr()
            if self.ordered is not None:
                d.ordered = self.ordered
                d.ordered_work = self.ordered_work.data_ptr()
            self._descs[key] = d
        return d

    def build_list(self, labels):
        """labels [N, CT * A] int32 -> self.list / self.state / self.map on the device."""
        assert labels.dtype == torch.int32 and labels.numel() == self.N * self.CT * self.A and labels.is_contiguous()
        check(_lib.load().mxdet_rpn_sparse_list(C.byref(self._desc()), ptr(labels), ptr(self.list), ptr(self.state),
                                                ptr(self.map), stream_ptr()), "rpn_sparse_list")

    def backward(self, P, t, tbits, gh, dP, accumulate, wt_out, wt_conv, dw_out, db_out, dw_conv, db_conv, parts=ALL, dt=None):
        """The parts of the head's backward named in `parts` (ZERO | DT | DTMAP | WGRAD | DGRAD | WGRAD_ORDERED), on the current
        stream. WGRAD_ORDERED (after plan_ordered()): the weight gradients with the bits of the dense grouped kernels.
        dt (DTMAP): dense [N,H,W,C] maps that receive the listed dt rows (zero elsewhere)."""
        d = self._desc(P, t, tbits, gh, dP, accumulate, dt)
        check(_lib.load().mxdet_rpn_sparse_backward(C.byref(d), ptr(self.list), ptr(self.state), ptr(self.map), ptr(wt_out),
                                                    ptr(wt_conv), ptr(self.dts), ptr(self.ghs), ptr(dw_out), ptr(db_out),
                                                    ptr(dw_conv), ptr(db_conv), parts, stream_ptr()), "rpn_sparse_backward")
