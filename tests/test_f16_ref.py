"""round_f16 (tests/f16_ref.py), the whole host model of what an f16 store holds, against torch's float32 -> float16 conversion: bit
for bit; and the f64 cells and the flag rule of the euclidean expansion on cases small enough to read."""
import numpy as np
import pytest

import f16_ref as F

torch = pytest.importorskip("torch")


def torch_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float16).to(torch.float32).numpy()


def same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def inputs():
    rng = np.random.default_rng(2025)
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)     # every finite non-negative f16 value
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)   # every tie between two of them (exact in f32)
    return {
        "uniform": rng.uniform(0, 1, 100_000).astype(np.float32),
        "normal": rng.normal(0, 100, 100_000).astype(np.float32),
        "subnormal": np.concatenate([rng.uniform(-6.2e-5, 6.2e-5, 50_000), rng.uniform(-1.2e-7, 1.2e-7, 10_000),
                                     [2.0**-24, 2.0**-25, 1.5 * 2.0**-25, 2.0**-26, 2.0**-14, 2.0**-14 - 2.0**-25, 1e-30, 1e-45]]).astype(np.float32),
        "ties": np.concatenate([mid, -mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))]),
        "top": np.array([65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 1e9, 3.4e38, np.inf, -65504.0, -65520.0, -np.inf], np.float32),
        "zeros": np.array([0.0, -0.0], np.float32),
        "nan": np.array([np.nan, -np.nan], np.float32),
        "representable": h,
    }


@pytest.mark.parametrize("name", ["uniform", "normal", "subnormal", "ties", "top", "zeros", "nan", "representable"])
def test_round_f16_is_torchs_conversion(name):
    x = inputs()[name]
    got, want = F.round_f16(x), torch_round(x)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    same_bits(got[m], want[m])
    if name == "nan":
        assert np.isnan(got).all()


def test_the_named_values():
    r = F.round_f16(np.array([1.00048828125, 1.00146484375, 65504.0, 65519.996, 65520.0, -65520.0], np.float32))   # ties: to even, down and up
    assert r[0] == np.float32(1.0) and r[1] == np.float32(1.001953125)
    assert r[2] == r[3] == np.float32(65504.0) and r[4] == np.inf and r[5] == -np.inf
    z = F.round_f16(np.array([0.0, -0.0, 1e-30, -1e-30], np.float32)).view(np.uint32)
    assert z[0] == 0 and z[1] == 0x80000000 and z[2] == 0 and z[3] == 0x80000000
    s = F.round_f16(np.array([2.0**-24, 2.0**-25, 1.5 * 2.0**-25, 3 * 2.0**-25], np.float32))   # the smallest subnormal, a tie to zero, above it, a tie up
    assert s[0] == np.float32(2.0**-24) and s[1] == 0 and s[2] == np.float32(2.0**-24) and s[3] == np.float32(2.0**-23)
    assert not F.FLUSH_SUBNORMALS
    assert not (F.round_f16(inputs()["normal"]).view(np.uint32) & 0x1FFF).any()   # an f16 value: 13 low mantissa bits are zero


def test_rounding_is_idempotent_and_keeps_f16_rows():
    for name, x in inputs().items():
        if name == "nan":
            continue
        once = F.round_f16(x)
        same_bits(F.round_f16(once), once)
    h = inputs()["representable"]
    same_bits(F.round_f16(h), h)
    same_bits(F.round_f16(-h), -h)


def test_shapes_and_empty_banks_pass_through():
    assert F.round_f16(np.zeros((0, 7), np.float32)).shape == (0, 7)
    x = np.random.default_rng(1).uniform(0, 1, (3, 5)).astype(np.float32)
    assert F.round_f16(x).shape == (3, 5)
    m = F.Model(2, 5)
    m.upsert([4], [x[:2]])
    same_bits(m.feats(4), F.round_f16(x[:2]))
    m.append([4, 9], [x[2:], x[:1]], keep="latest")
    same_bits(m.feats(4), F.round_f16(x[1:]))
    same_bits(m.feats(9), F.round_f16(x[:1]))


def test_cells_f64_marks_absent_rows_and_measures_both_ways():
    q = [np.array([[3.0, 0.0]], np.float32), np.zeros((0, 2), np.float32)]
    s = [np.array([[0.0, 4.0], [0.0, 0.0]], np.float32)]
    c = F.cells_f64("cosine", q, s, 2)
    assert c.shape == (2, 2, 1, 2) and c[0, 0, 0, 0] == 0.0
    assert np.isnan(c[0, 0, 0, 1]) and np.isnan(c[0, 1]).all() and np.isnan(c[1]).all()
    e = F.cells_f64("euclidean", q, s, 2)
    assert e[0, 0, 0, 0] == 5.0 and e[0, 0, 0, 1] == 3.0 and np.isnan(e[0, 1]).all() and np.isnan(e[1]).all()
    r = F.flag_ratio(q, s, 2)
    assert r[0, 0, 0, 0] == 1.0 and r[0, 0, 0, 1] == 1.0
    assert F.flag_ratio(q[:1], q[:1], 2)[0, 0, 0, 0] == 0.0   # a duplicate: below any rho


def test_rho_is_the_frame_paths_rule_on_the_padded_length():
    assert F.rho(32) == F.rho(1) == np.float32(5e-3) * np.sqrt(np.float32(32))
    assert F.rho(33) == F.rho(64) and abs(float(F.rho(512)) - 0.11313708) < 1e-7
    assert F.rho(40000) >= 1.0 > F.rho(39968)
