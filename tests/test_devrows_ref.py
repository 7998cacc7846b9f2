"""tests/devrows_ref.py against torch's CPU conversions and against the header's words."""
import numpy as np
import pytest

import devrows_ref as ref

ALL = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def same_values(got, want):
    """Bit for bit, except that NaNs compare as NaN-ness plus sign."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w)
    assert np.array_equal(g[~nan_g], w[~nan_w])
    assert np.array_equal(g[nan_g] >> 31, w[nan_w] >> 31)


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_widen_is_torchs_conversion_over_every_pattern(name):
    torch = pytest.importorskip("torch")
    dt = getattr(torch, name)
    want = torch.from_numpy(ALL.view(np.int16).copy()).view(dt).to(torch.float32).numpy()
    got = ref.widen_f16(ALL) if name == "float16" else ref.widen_bf16(ALL)
    assert got.dtype == np.float32
    same_values(got, want)


def test_widen_f16_is_numpys_conversion_and_keeps_nan_payloads():
    want = ALL.view(np.float16).astype(np.float32)
    same_values(ref.widen_f16(ALL), want)
    assert ref.widen_f16(np.array([0x7C01, 0xFE00, 0x0001, 0x8001, 0x7BFF], np.uint16)).view(np.uint32).tolist() == [
        0x7F802000, 0xFFC00000, 0x33800000, 0xB3800000, 0x477FE000]
    assert ref.widen_bf16(np.array([0x7F81, 0x8000, 0x0001], np.uint16)).view(np.uint32).tolist() == [0x7F810000, 0x80000000, 0x00010000]
    x = np.array([1.5, -0.0], np.float32)
    assert ref.widen(x, ref.ELEM_F32).view(np.uint32).tolist() == x.view(np.uint32).tolist()


def test_row_table():
    N = ref.NONE
    assert ref.row_table([2, 0, 3, 1], None, 4).tolist() == [0, 1, N, N, N, N, N, N, 2, 3, 4, N, 5, N, N, N]
    assert ref.row_table([2, 0, 3, 1], [9, 9, 0, 7, 2, 5], 4).tolist() == [9, 9, N, N, N, N, N, N, 0, 7, 2, N, 5, N, N, N]
    assert ref.row_table([], None, 4).tolist() == []
    assert ref.row_table([1, 1], [3, 3], 1).tolist() == [3, 3]


def test_span_and_wide_rows():
    assert ref.span_bytes(1, 1000, 33, ref.ELEM_F16) == 66
    assert ref.span_bytes(10, 40, 33, ref.ELEM_F32) == (9 * 40 + 33) * 4
    assert ref.span_bytes(3, 100, 100, ref.ELEM_BF16) == 600
    F32, BF, F16 = ref.ELEM_F32, ref.ELEM_BF16, ref.ELEM_F16
    assert [ref.wide_bytes(s, d, 100) for s in (F32, F16) for d in (F32, F16)] == [16, 8, 8, 4]
    assert ref.wide_bytes(BF, F32, 33) == 0 and ref.wide_bytes(F32, F32, 5) == 0 and ref.wide_bytes(F32, BF, 5) == 8
    # rows of 33 f16 elements, stride 33: every second row starts on a 4-byte boundary
    assert ref.wide_rows(0x1000, 33, [0, 1, 2, 3, ref.NONE, 4], F16, F16, 33) == 3
    assert ref.wide_rows(0x1002, 33, [0, 1, 2, 3], F16, F16, 33) == 2
    assert ref.wide_rows(0x1000, 33, [0, 1, 2, 3], F32, F16, 33) == 2
    assert ref.wide_rows(0x1000, 33, [0, 1, 2, 3], F32, F32, 33) == 0
