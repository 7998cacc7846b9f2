"""Feature rows read from device memory on the MI355X (similari_amd.devrows.DeviceRowsStore over include/similari_devrows.h).

The contract admits no tolerance: a *_dev call returns, and leaves in the store, exactly the bits the host call returns and leaves
when it is fed widen(x) for every source element.  So every test here runs a twin — one store (or call) fed from device memory, one
fed tests/devrows_ref.widen of the same source from the host — and compares every array bit for bit.  The cells of a tapped search
carry the norms: a norm summed in another order than the host-fed kernel's shows there.  sa_store_devrows_last proves which load
route the rows took.  Device memory comes from tests/hipmem.py; every block is unregistered and freed in a finally.

The twin is held at D up to 1024, past the first step of every loop of the pad kernel (a 16-bit store steps by 128 elements, an f32
store with D % 4 == 0 by 256).  Beside it every upsert is held against numpy for its finite rows: fetch returns exactly the store's
rounding of widen(bits), and the tapped cells of a cosine store lie within the suite's 1e-5 of f64 on those rows."""
import contextlib
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bf16_ref
import devrows_ref as ref
import f16_ref
import hipmem
from similari_amd import abi, attrs as A, devrows as DR
from similari_amd.devrows import DeviceRows, DeviceRowsStore
from similari_amd.engine import Engine, EngineError
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32

pytestmark = pytest.mark.gpu
u16, u32, u64 = np.uint16, np.uint32, np.uint64
F32, BF16, F16 = SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16
ELEMS = [F32, F16, BF16]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
STORES = [(F32, "cosine"), (F32, "euclidean"), (BF16, "cosine"), (F16, "cosine"), (F16, "euclidean")]
K, KP, T = 3, 4, 21
FAR = 3.0e38   # above every distance


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


# ---- sources -------------------------------------------------------------------------------------
def make_source(rng, n_rows, D, elem):
    """[n_rows][D] source elements as they lie in device memory: f32 values, or uint16 bit patterns of f16 / bf16.  Both signs and
    thirteen binades; row 1 in the f16 subnormal range, +-0 in row 2, +-inf in row 3, NaNs in row 4; an f32 source also carries the
    three values around the f16 overflow threshold in row 5."""
    x = rng.uniform(-1, 1, (n_rows, D)).astype(np.float32)
    x *= np.float32(2.0) ** rng.integers(-6, 7, (n_rows, 1)).astype(np.float32)
    if n_rows > 5:
        x[1] = rng.uniform(-6e-5, 6e-5, D).astype(np.float32)
        x[2, 0], x[2, 1] = 0.0, -0.0
        x[3, D - 1], x[3, 0] = np.inf, -np.inf
        x[4, D // 2], x[4, 0] = np.nan, -np.nan
        if elem == F32:
            x[5, :3] = [65504.0, 65519.0, -65520.0]
    if elem == F32:
        return x
    if elem == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(u16)
    return (x.view(u32) >> 16).astype(u16)   # any 16 bits are a bf16 value


def lay_rows(bits, stride, offset):
    """The image of a block that holds `bits` rows `stride` elements apart from element `offset` on and ENDS with the last row's last
    element; every element that is not a row's is a NaN pattern, so a read past a row's end would show in a norm."""
    n, D = bits.shape
    img = np.full(offset + (n - 1) * stride + D, 0x7FFF if bits.dtype == u16 else np.nan, bits.dtype)
    for r in range(n):
        img[offset + r * stride: offset + r * stride + D] = bits[r]
    return img


@contextlib.contextmanager
def device_block(engine, image, device=0, register=True):
    """image (a numpy array) in device memory of exactly its size, registered for the body -> its device address."""
    ptr = hipmem.malloc(image.nbytes)
    try:
        hipmem.upload(ptr, image)
        if register:
            engine.register_device_block(ptr, image.nbytes, device)
        yield ptr
    finally:
        if register:
            engine.unregister_device_block(ptr)
        hipmem.free(ptr)


def banks_of(rows_f32, n_obs, index=None):
    """The per-track host arrays of a call whose observation j is row index[j] (or j) of rows_f32."""
    out, off = [], 0
    for m in n_obs:
        take = [off + k if index is None else int(index[off + k]) for k in range(int(m))]
        out.append(rows_f32[take].reshape(int(m), rows_f32.shape[1]))
        off += int(m)
    return out


def ragged(rng, n):
    n_obs = rng.integers(0, K + 1, n).astype(u32)
    n_obs[:4] = [0, 1, 2, 3]   # every count, a track without any among them
    return n_obs


# ---- comparisons ---------------------------------------------------------------------------------
def same_out(a, b):
    """Two tuples of arrays (or None): dtype, shape and every bit."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), i
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, i
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), "output %d differs" % i


def same_store(a, b):
    ids = a.order()
    assert len(a) == len(b) and np.array_equal(ids, b.order())
    same_out(a.fetch_raw(ids), b.fetch_raw(ids))


def same_search(rng, a, b, D, nq=5):
    """Host-fed queries on both stores, tapped: out_n, winners, weights and every cell (which carry the stored norms)."""
    q_ids = np.arange(1000, 1000 + nq, dtype=u64)
    q = [rng.uniform(-1, 1, (int(m), D)).astype(np.float32) for m in rng.integers(1, K + 1, nq)]
    same_out(a.search_raw(q_ids, q, 3, FAR, tap=True), b.search_raw(q_ids, q, 3, FAR, tap=True))


def twin(engine, kind, D, elem):
    return DeviceRowsStore(engine, kind, D, K, elem), DeviceRowsStore(engine, kind, D, K, elem)


ROUND = {F32: lambda x: np.ascontiguousarray(x, np.float32), F16: f16_ref.round_f16, BF16: bf16_ref.round_bf16}


def against_numpy(store, kind, D, store_elem, ids, banks):
    """The finite rows of a store that was fed `banks` (widen of the source), without the twin: fetch returns the store's rounding
    of each, bit for bit; a cosine store's tapped cells lie within 1e-5 of f64 on the rounded rows (f16_ref.cells_f64, the gate of
    test_gpu_bf16 / test_gpu_f16).  A row is finite if its rounding is: make_source's +-inf row, its NaN row and, from an f32
    source into an f16 store, its row around 65520 are left to the twin.  -> the number of rows checked"""
    with np.errstate(over="ignore", invalid="ignore"):
        want = [ROUND[store_elem](f) for f in banks]
    n_obs, got, _ = store.fetch_raw(ids)
    live = np.zeros((len(ids), K), bool)
    for t, w in enumerate(want):
        assert n_obs[t] == len(w)
        live[t, : len(w)] = np.isfinite(w).all(axis=1)
        m = live[t, : len(w)]
        assert np.array_equal(got[t, : len(w)][m].view(u32), w[m].view(u32)), "track %d" % t
    if kind == "cosine":
        rng = np.random.default_rng(D)
        q = [rng.uniform(-1, 1, (m, D)).astype(np.float32) for m in (1, K, 2)]
        cells = store.search_raw(np.arange(2000, 2003, dtype=u64), q, 3, FAR, tap=True)[3]
        with np.errstate(over="ignore", invalid="ignore"):
            f64 = f16_ref.cells_f64("cosine", [ROUND[store_elem](x) for x in q], want, K)
        a, b = cells[:, :, live], f64[:, :, live]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        both = ~np.isnan(b)
        err = float(np.abs(a[both].astype(np.float64) - b[both]).max())
        print("D = %d, %s store: max |cell - f64 of the rounded rows| = %.3g over %d cells" % (D, NAME[store_elem], err, int(both.sum())))
        assert both.sum() >= 5 * live.sum() and err <= 1e-5
    return int(live.sum())


def upsert_twin(engine, rng, store_elem, kind, D, src_elem, stride=None, offset=0, index_of=None):
    """T ragged banks through upsert_rows and through upsert(widen(rows)) -> (stats, expected wide rows, total rows)."""
    ids = np.arange(1, T + 1, dtype=u64)
    n_obs = ragged(rng, T)
    total = int(n_obs.sum())
    n_rows = total + 3
    bits = make_source(rng, n_rows, D, src_elem)
    index = None if index_of is None else index_of(total, n_rows)
    stride = D if stride is None else stride
    img = lay_rows(bits, stride, offset)
    eb = ref.ELEM_BYTES[src_elem]
    a, b = twin(engine, kind, D, store_elem)
    try:
        with device_block(engine, img) as ptr:
            base = ptr + offset * eb
            a.upsert_rows(ids, n_obs, DeviceRows(base, n_rows, stride, src_elem, index))
            st = a.devrows_stats()
        banks = banks_of(ref.widen(bits, src_elem), n_obs, index)
        b.upsert(ids, banks)
        same_store(a, b)
        same_search(rng, a, b, D)
        assert against_numpy(a, kind, D, store_elem, ids, banks) >= total - 4 > 0
        table = ref.row_table(n_obs, index, KP)
        assert st["rows"] == total and st["src_bytes"] == total * D * eb
        want_wide = ref.wide_rows(base, stride, table, src_elem, store_elem, D)
        assert st["wide_rows"] == want_wide
        return st, want_wide, total
    finally:
        a.close()
        b.close()


# ---- 1. upsert, every pairing --------------------------------------------------------------------
@pytest.mark.parametrize("src_elem", ELEMS, ids=lambda e: "from_" + NAME[e])
@pytest.mark.parametrize("store_elem,kind", STORES, ids=lambda v: NAME.get(v, v) if isinstance(v, int) else v)
def test_upsert_from_device_rows_leaves_the_host_calls_bits(engine, store_elem, kind, src_elem):
    """D = 5: odd, inside one 32-chunk; 33: one past a chunk; 64: D == Dp; 100: the f32 store's D % 4 == 0 norm order with a row
    that ends inside the fourth chunk."""
    rng = np.random.default_rng(1000 + 10 * store_elem + src_elem)
    for D in (5, 33, 64, 100):
        upsert_twin(engine, rng, store_elem, kind, D, src_elem)


@pytest.mark.parametrize("src_elem", ELEMS, ids=lambda e: "from_" + NAME[e])
@pytest.mark.parametrize("store_elem,kind", STORES, ids=lambda v: NAME.get(v, v) if isinstance(v, int) else v)
def test_upsert_from_device_rows_at_widths_beyond_one_step(engine, store_elem, kind, src_elem):
    """D = 129: the second step of a 16-bit store (k += 128) is one pair whose high half is padding, and the wide load's k + 1 < D
    guard falls on a later step; 260: the second step of the f32 store's float4 route (k += 256) has one live lane; 512 and 1024:
    full steps at the re-ID widths, the norm summed over four and eight steps of a 16-bit store."""
    rng = np.random.default_rng(1500 + 10 * store_elem + src_elem)
    for D in (129, 260, 512, 1024):
        upsert_twin(engine, rng, store_elem, kind, D, src_elem)


# ---- 2. address forms ----------------------------------------------------------------------------
FORMS = [(F32, "cosine", 100), (F16, "euclidean", 33), (F32, "cosine", 260), (F16, "euclidean", 513)]


def pad16(D, eb):
    """The smallest stride >= D whose rows are a multiple of 16 bytes apart."""
    per = 16 // eb
    return (D + per - 1) // per * per


@pytest.mark.parametrize("src_elem", [F16, F32], ids=lambda e: "from_" + NAME[e])
@pytest.mark.parametrize("store_elem,kind,D", FORMS, ids=lambda v: NAME.get(v, v) if isinstance(v, int) and v < 3 else str(v))
def test_address_forms(engine, store_elem, kind, D, src_elem):
    """The same bits as the host twin from every address form; which rows took the wide load follows from their addresses alone.
    The f32 store at D = 100 is the case that catches a norm summed in the wrong order."""
    rng = np.random.default_rng(2000 + 10 * store_elem + src_elem)
    eb = ref.ELEM_BYTES[src_elem]
    # (a) base 16-byte aligned (hipMalloc's), rows a multiple of 16 bytes apart: every row is read wide
    st, _, total = upsert_twin(engine, rng, store_elem, kind, D, src_elem, stride=pad16(D, eb))
    assert st["wide_rows"] == st["rows"] == total
    # (b) the same, one element past the aligned address: no row is
    st, _, _ = upsert_twin(engine, rng, store_elem, kind, D, src_elem, stride=pad16(D, eb), offset=1)
    assert st["wide_rows"] == 0
    # (c) row_stride == D.  An odd D alternates between the two alignments (D = 33: a 16-bit source row is 66 bytes and its wide
    # load 4, an f32 source row 132 bytes and its wide load 8; D = 513: 1026 and 2052 bytes): rows 0, 2, 4, .. are wide.  With
    # these even D every row is (D = 100: 200 and 400 bytes, loads of 8 and 16; D = 260: 520 and 1040 bytes).
    # (f) This block also ends exactly at the last row's last byte, as every block of these tests does.
    st, want, total = upsert_twin(engine, rng, store_elem, kind, D, src_elem, stride=D)
    assert want == ((total + 1) // 2 if D % 2 else total)
    if D % 2:
        assert 0 < st["wide_rows"] < st["rows"]
    # (d) row_stride = D + 3
    upsert_twin(engine, rng, store_elem, kind, D, src_elem, stride=D + 3)

    # (e) an index that is reversed, skips rows and names one row for two observations
    def index_of(total, n_rows):
        ix = np.arange(n_rows - 1, n_rows - 1 - total, -1).astype(u32)   # reversed; rows 0 and 1 are skipped
        ix[1] = ix[0]                                                     # one row for two observations (and its neighbour skipped)
        return ix

    upsert_twin(engine, rng, store_elem, kind, D, src_elem, stride=D + 1, index_of=index_of)


# ---- 3. append -----------------------------------------------------------------------------------
@pytest.mark.parametrize("store_elem,kind,D,src_elem", [(F32, "cosine", 100, F16), (F16, "euclidean", 33, F32), (BF16, "cosine", 33, BF16),
                                                        (F16, "euclidean", 512, F16), (F32, "cosine", 512, BF16)],
                         ids=["f16_into_f32", "f32_into_f16", "bf16_into_bf16", "f16_into_f16_512", "bf16_into_f32_512"])
def test_append_from_device_rows(engine, store_elem, kind, D, src_elem):
    rng = np.random.default_rng(3000 + store_elem)
    a, b = twin(engine, kind, D, store_elem)
    try:
        ids0 = np.arange(1, 11, dtype=u64)
        start = [rng.uniform(-1, 1, (int(m), D)).astype(np.float32) for m in rng.integers(0, K + 1, 10)]
        a.upsert(ids0, start)
        b.upsert(ids0, start)
        calls = [("best", 2, np.array([3, 99, 5, 1, 7], u64), np.array([2, 2, 0, 3, 1], u32)),       # 99 is unknown: created; 5 is left alone
                 ("latest", None, np.array([99, 2, 98, 4], u64), np.array([3, 1, 0, 2], u32))]       # 98: created without a row
        for keep, cap, ids, n_obs in calls:
            total = int(n_obs.sum())
            bits = make_source(rng, total + 2, D, src_elem)
            index = rng.permutation(total + 2)[:total].astype(u32)
            quality = rng.uniform(0, 1, total).astype(np.float32)
            with device_block(engine, lay_rows(bits, D + 1, 1)) as ptr:
                a.append_rows(ids, n_obs, DeviceRows(ptr + ref.ELEM_BYTES[src_elem], total + 2, D + 1, src_elem, index), quality, cap, keep)
            assert a.devrows_stats()["rows"] == total
            qs, off = [], 0
            for m in n_obs:
                qs.append(quality[off:off + int(m)])
                off += int(m)
            b.append(ids, banks_of(ref.widen(bits, src_elem), n_obs, index), qs, keep, cap)
            same_store(a, b)
            same_search(rng, a, b, D)
        for s in (a, b):
            s.merge({1: [2], 3: [4, 99]}, keep="best", capacity=2)
        same_store(a, b)
        same_search(rng, a, b, D)
    finally:
        a.close()
        b.close()


# ---- 4. search -----------------------------------------------------------------------------------
def filled_store(engine, rng, kind, D, elem, full=False):
    s = DeviceRowsStore(engine, kind, D, K, elem)
    ids = np.arange(1, T + 1, dtype=u64)
    n_obs = np.full(T, K, u32) if full else ragged(rng, T)
    s.upsert(ids, [rng.uniform(-1, 1, (int(m), D)).astype(np.float32) for m in n_obs])
    s.set_attrs(ids, ids % 3, np.arange(T) * 10, np.arange(T) * 10 + 5)
    return s


@pytest.mark.parametrize("store_elem,kind,D,src_elem", [(F32, "cosine", 100, F16), (F16, "euclidean", 33, BF16), (BF16, "cosine", 64, F32),
                                                        (F16, "euclidean", 512, F16), (F32, "cosine", 512, BF16)],
                         ids=["f16_into_f32", "bf16_into_f16", "f32_into_bf16", "f16_into_f16_512", "bf16_into_f32_512"])
def test_search_with_queries_from_device_rows(engine, store_elem, kind, D, src_elem):
    rng = np.random.default_rng(4000 + store_elem)
    s = filled_store(engine, rng, kind, D, store_elem)
    try:
        Q = 6
        q_ids = np.arange(500, 500 + Q, dtype=u64)
        q_n_obs = np.array([2, 0, 3, 1, 3, 2], u32)   # one query without an observation
        total = int(q_n_obs.sum())
        bits = make_source(rng, total + 1, D, src_elem)
        index = rng.permutation(total + 1)[:total].astype(u32)
        q_host = banks_of(ref.widen(bits, src_elem), q_n_obs, index)
        q_attrs = A.pack_attrs(q_ids % 3, np.full(Q, 1000), np.full(Q, 1005))
        rule = A.compat(same_key=True, disjoint=True)
        with device_block(engine, lay_rows(bits, D + 2, 0)) as ptr:
            rows = DeviceRows(ptr, total + 1, D + 2, src_elem, index)
            same_out(s.search_rows_raw(q_ids, q_n_obs, rows, 3, FAR, tap=True), s.search_raw(q_ids, q_host, 3, FAR, tap=True))
            assert s.devrows_stats()["rows"] == total
            same_out(s.search_rows_raw(q_ids, q_n_obs, rows, 3, FAR, tap=True, compat=rule, q_attrs=q_attrs),
                     s.search_raw(q_ids, q_host, 3, FAR, tap=True, compat=rule, q_attrs=q_attrs))
            same_out(s.search_rows_raw(q_ids, q_n_obs, rows, 3, FAR, vote="bestfit", tap=True), s.search_bestfit_raw(q_ids, q_host, 3, FAR, tap=True))
            got = s.search_rows_raw(q_ids, q_n_obs, rows, 3, FAR, vote="bestfit", tap=True, compat=rule, q_attrs=q_attrs)
            same_out(got, s.search_bestfit_raw(q_ids, q_host, 3, FAR, tap=True, compat=rule, q_attrs=q_attrs))
            assert got[0].sum() > 0 and got[2] is not None   # groups survived the rule, and out_track was written
            assert s.search_rows(q_ids, q_n_obs, rows, 3, FAR) == s.search_topn(q_ids, q_host, 3, FAR)
            assert s.search_rows(q_ids, q_n_obs, rows, 3, FAR, vote="bestfit") == s.search_bestfit(q_ids, q_host, 3, FAR)
            # Q = 0
            none = np.zeros(0, u64)
            same_out(s.search_rows_raw(none, np.zeros(0, u32), rows, 3, FAR), s.search_raw(none, [], 3, FAR))
            # an empty store: outputs zeroed
            with DeviceRowsStore(engine, kind, D, K, store_elem) as empty:
                got = empty.search_rows_raw(q_ids, q_n_obs, rows, 3, FAR, vote="bestfit")
                same_out(got, empty.search_bestfit_raw(q_ids, q_host, 3, FAR))
                assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
    finally:
        s.close()


def test_a_pool_rerun_reuses_the_padded_queries(engine):
    """Fresh stores (a first pool holds 256 blocks), 24 queries with ids outside the store against 21 full banks, max_distance above
    every distance, min_votes 1: 504 surviving groups, so each call reruns once — and returns the same bits."""
    rng = np.random.default_rng(4500)
    D, Q = 33, 24
    a = filled_store(engine, np.random.default_rng(4502), "euclidean", D, F16, full=True)
    b = filled_store(engine, np.random.default_rng(4502), "euclidean", D, F16, full=True)
    try:
        same_store(a, b)
        q_ids = np.arange(500, 500 + Q, dtype=u64)
        q_n_obs = np.full(Q, K, u32)
        bits = make_source(rng, Q * K, D, F16)
        bits = np.where(np.isfinite(ref.widen(bits, F16)), bits, u16(0x3C00))
        with device_block(engine, lay_rows(bits, D, 0)) as ptr:
            got = a.search_rows_raw(q_ids, q_n_obs, DeviceRows(ptr, Q * K, D, F16), 3, FAR, min_votes=1, tap=True)
        want = b.search_raw(q_ids, banks_of(ref.widen(bits, F16), q_n_obs), 3, FAR, min_votes=1, tap=True)
        assert a.last_stats()["groups"] == b.last_stats()["groups"] == Q * T == 504
        assert a.last_stats()["reruns"] == 1 and b.last_stats()["reruns"] == 1
        same_out(got, want)
    finally:
        a.close()
        b.close()


# ---- 5. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_the_store_as_it_was(engine):
    """Host checks that launch nothing.  Every address handed over lies inside this test's own allocations."""
    rng = np.random.default_rng(5000)
    D, n_rows = 33, 12
    s = filled_store(engine, rng, "cosine", D, F16)
    bits = make_source(rng, n_rows, D, F16)
    ids = np.array([1, 2, 77], u64)
    n_obs = np.array([2, 1, 3], u32)   # 6 observations
    total = 6

    def state():
        return len(s), s.order().tobytes(), [x.tobytes() for x in s.fetch_raw(s.order())]

    before = state()
    prm = DR.sa_topn_params(3, 1, FAR, math.inf)
    try:
        with device_block(engine, lay_rows(bits, D, 0)) as ptr, device_block(engine, lay_rows(bits, D, 0), register=False) as loose, \
                device_block(engine, lay_rows(bits, D, 0), device=1) as other:
            good = DeviceRows(ptr, n_rows, D, F16)
            small = good.struct()
            small.struct_size = 39

            def search_raw_call(vote, rule, qa, track):
                out_n, win, wt = np.zeros(3, u32), np.zeros((3, 3), u64), np.zeros((3, 3), np.float64)
                trk = np.zeros((3, 3), u64) if track else None
                st = good.struct()
                p = lambda x, t: None if x is None else x.ctypes.data_as(C.POINTER(t))   # noqa: E731
                s._chk(s.lib.sa_store_search_dev(s.h, C.byref(prm), vote, None if rule is None else C.byref(rule), 3, p(ids, C.c_uint64),
                                                 p(n_obs, C.c_uint32), C.byref(st), p(qa, DR.sa_track_attrs), p(out_n, C.c_uint32),
                                                 p(win, C.c_uint64), p(trk, C.c_uint64), p(wt, C.c_double), None))

            rule = A.compat(same_key=True).struct()
            qa = A.pack_attrs([0, 1, 2], [0, 0, 0], [5, 5, 5])
            cases = [
                ("null rows", lambda: None),
                ("null rows.base", lambda: DeviceRows(0, n_rows, D, F16)),
                ("struct_size", lambda: small),
                ("unknown element type", lambda: DeviceRows(ptr, n_rows, D, 7)),
                ("not aligned", lambda: DeviceRows(ptr + 1, n_rows - 1, D, F16)),                      # an odd base for f16 elements
                ("row_stride", lambda: DeviceRows(ptr, n_rows, D - 1, F16)),
                ("n_rows", lambda: DeviceRows(ptr, 0xFFFFFFFF, D, F16)),
                ("index", lambda: DeviceRows(ptr, n_rows, D, F16, [0, 1, 2, n_rows, 3, 4])),
                ("observations", lambda: DeviceRows(ptr, total - 1, D, F16)),                          # sum n_obs > n_rows, no index
                ("not inside one block", lambda: DeviceRows(ptr + 2, n_rows, D, F16)),                  # the span ends one element past the block
                ("not inside one block", lambda: DeviceRows(loose, n_rows, D, F16)),                    # never registered
                ("registered for device 1", lambda: DeviceRows(other, n_rows, D, F16)),
            ]
            for word, make in cases:
                for call in (lambda r: s.upsert_rows(ids, n_obs, r), lambda r: s.append_rows(ids, n_obs, r),
                             lambda r: s.search_rows_raw(ids, n_obs, r, 3, FAR)):
                    with pytest.raises(EngineError) as ex:
                        call(make())
                    assert ex.value.code == abi.SA_ERR_BAD_ARG and word in str(ex.value), (word, str(ex.value))
                    assert state() == before, word
            for word, call in [("out_track", lambda: search_raw_call(DR.SA_VOTE_TOPN, None, None, True)),
                               ("come together", lambda: search_raw_call(DR.SA_VOTE_TOPN, rule, None, False)),
                               ("come together", lambda: search_raw_call(DR.SA_VOTE_BESTFIT, None, qa, True)),
                               ("unknown vote", lambda: search_raw_call(7, None, None, False))]:
                with pytest.raises(EngineError) as ex:
                    call()
                assert ex.value.code == abi.SA_ERR_BAD_ARG and word in str(ex.value), (word, str(ex.value))
                assert state() == before, word
            # what the host calls refuse is refused with the same code: more observations than a bank holds, an id twice
            with pytest.raises(EngineError) as ex:
                s.upsert_rows(ids, np.array([K + 1, 1, 1], u32), good)
            assert ex.value.code == abi.SA_ERR_BAD_ARG and "observations" in str(ex.value)
            with pytest.raises(EngineError) as ex:
                s.search_rows_raw(np.array([5, 5], u64), np.array([1, 1], u32), good, 3, FAR)
            assert ex.value.code == abi.SA_ERR_BAD_ARG and "twice" in str(ex.value)
            assert state() == before
            # the next valid calls succeed
            out = s.search_rows_raw(ids, n_obs, good, 3, FAR)
            assert out[0].sum() > 0
            s.upsert_rows(ids, n_obs, good)
            assert len(s) == T + 1 and s.devrows_stats()["rows"] == total
            got = s.fetch_raw(np.array([77], u64))
            assert got[0][0] == 3 and got[1][0].tobytes() == ref.widen(bits[3:6], F16).tobytes()
    finally:
        s.close()


def test_stats_are_zero_before_the_first_call(engine):
    with DeviceRowsStore(engine, "cosine", 8, 1, F32) as s:
        assert s.devrows_stats() == {"rows": 0, "wide_rows": 0, "src_bytes": 0}
        s.upsert_rows(np.array([4], u64), np.array([0], u32), None)   # a bank without rows reads nothing and needs no descriptor
        assert len(s) == 1 and s.devrows_stats() == {"rows": 0, "wide_rows": 0, "src_bytes": 0}


# ---- 6. the tensor interface ---------------------------------------------------------------------
def test_rows_of_a_torch_tensor_on_the_gpu():
    """register_tensor, DeviceRows.from_tensor of a column slice of an fp16 and a bf16 tensor, upsert_rows and search_rows against a
    host-fed twin.  Runs tests/devrows_child.py: torch's HIP context wants to be the first one of its process."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devrows_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE-ROWS-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
