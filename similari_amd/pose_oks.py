"""ctypes mirror of include/similari_pose_oks.h: object keypoint similarity (OKS) as the metric of a point bank's votes, beside the
default mean inverted Mahalanobis cost.

    bank = PoseBank(engine, points=17, metric=OksMetric(COCO_SIGMAS))     # every vote of this bank is by OKS; threshold defaults to 0.3
    trk = KeypointSort(engine, points=17, metric=OksMetric(COCO_SIGMAS))
    set_metric(bank, None)                                                # back to Mahalanobis: the launches and bits of before
    get_metric(bank)                                                      # None, or the OksMetric
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .points import POINTS

u32 = C.c_uint32
P = C.POINTER
SA_POSE_METRIC_MAHALANOBIS, SA_POSE_METRIC_OKS = 0, 1
OKS_DEFAULT_THRESHOLD = 0.3   # the reference's DEFAULT_SORT_IOU_THRESHOLD (sort.rs): w <= 1 under OKS, so the 1.0 of the Mahalanobis vote matches nothing
COCO_SIGMAS = (.026, .025, .025, .035, .035, .079, .079, .072, .072, .062, .062, .107, .107, .087, .087, .089, .089)


class sa_pose_metric(C.Structure):
    _fields_ = [("struct_size", u32), ("kind", u32), ("n_sigmas", u32), ("reserved", u32), ("sigmas", P(C.c_float))]


# ---- prototypes of every symbol include/similari_pose_oks.h declares -----------------------------
PROTOTYPES = {
    "sa_pose_metric_default": (None, [P(sa_pose_metric)]),
    "sa_points_set_metric": (C.c_int, [POINTS, P(sa_pose_metric)]),
    "sa_points_get_metric": (C.c_int, [POINTS, P(u32), P(C.c_float)]),
}


def bind(lib: C.CDLL) -> C.CDLL:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    return lib


def _bound(lib):
    if not getattr(lib, "_sa_pose_oks_bound", False):
        bind(lib)
        lib._sa_pose_oks_bound = True
    return lib


class OksMetric:
    """Object keypoint similarity with one sigma per point of the bank (each finite and > 0), as f32."""

    def __init__(self, sigmas=COCO_SIGMAS):
        self.sigmas = np.ascontiguousarray(sigmas, np.float32).reshape(-1)

    def __eq__(self, other):
        return isinstance(other, OksMetric) and np.array_equal(self.sigmas.view(np.uint32), other.sigmas.view(np.uint32))

    def __repr__(self):
        return f"OksMetric({self.sigmas.tolist()})"


def default_threshold(metric, threshold, otherwise=1.0):
    """The diagonal of a vote whose caller gave none: 0.3 under an OksMetric, the present default otherwise."""
    if threshold is not None:
        return threshold
    return OKS_DEFAULT_THRESHOLD if isinstance(metric, OksMetric) else otherwise


def set_metric(bank, metric) -> None:
    """metric: an OksMetric, or None for the Mahalanobis metric.  bank: a PointBank (or a tracker's bank()).  A refused call raises and
    leaves the previous metric."""
    lib = _bound(bank.lib)
    m = sa_pose_metric()
    lib.sa_pose_metric_default(C.byref(m))
    if metric is not None:
        m.kind, m.n_sigmas = SA_POSE_METRIC_OKS, len(metric.sigmas)
        m.sigmas = metric.sigmas.ctypes.data_as(P(C.c_float))
    bank._chk(lib.sa_points_set_metric(bank.h, C.byref(m)))
    bank.metric = metric


def get_metric(bank):
    """-> None (Mahalanobis) or the bank's OksMetric, as the library holds it."""
    lib = _bound(bank.lib)
    kind = u32()
    sig = np.zeros(bank.P, np.float32)
    bank._chk(lib.sa_points_get_metric(bank.h, C.byref(kind), sig.ctypes.data_as(P(C.c_float))))
    return OksMetric(sig) if kind.value == SA_POSE_METRIC_OKS else None
