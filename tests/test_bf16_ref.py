"""round_bf16 (tests/bf16_ref.py), the whole host model of a bf16 store, against torch's float32 -> bfloat16 conversion: bit for bit."""
import numpy as np
import pytest

import bf16_ref as B

torch = pytest.importorskip("torch")


def torch_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def inputs():
    rng = np.random.default_rng(2024)
    up = np.array([0x3FFFFFFF], np.uint32).view(np.float32)   # 1.9999999: rounds up into the next binade (2.0)
    return {
        "uniform": rng.uniform(0, 1, 100_000).astype(np.float32),
        "normal": rng.normal(0, 100, 100_000).astype(np.float32),
        "ties": np.array([1.00390625, 1.01171875, -1.00390625, -1.01171875], np.float32),
        "zeros": np.array([0.0, -0.0], np.float32),
        "binade": np.concatenate([up, -up, np.array([255.9999], np.float32)]),
    }


@pytest.mark.parametrize("name", ["uniform", "normal", "ties", "zeros", "binade"])
def test_round_bf16_is_torchs_conversion(name):
    x = inputs()[name]
    same_bits(B.round_bf16(x), torch_round(x))


def test_the_named_values():
    r = B.round_bf16(np.array([1.00390625, 1.01171875], np.float32))   # ties: to the even neighbour, down and up
    assert r[0] == np.float32(1.0) and r[1] == np.float32(1.015625)
    z = B.round_bf16(np.array([0.0, -0.0], np.float32)).view(np.uint32)
    assert z[0] == 0 and z[1] == 0x80000000
    up = np.array([0x3FFFFFFF], np.uint32).view(np.float32)
    assert B.round_bf16(up)[0] == np.float32(2.0)
    assert not (B.round_bf16(inputs()["normal"]).view(np.uint32) & 0xFFFF).any()   # a bf16 value: the lower half is zero


def test_rounding_is_idempotent():
    for x in inputs().values():
        once = B.round_bf16(x)
        same_bits(B.round_bf16(once), once)


def test_shapes_and_empty_banks_pass_through():
    assert B.round_bf16(np.zeros((0, 7), np.float32)).shape == (0, 7)
    x = np.random.default_rng(1).uniform(0, 1, (3, 5)).astype(np.float32)
    assert B.round_bf16(x).shape == (3, 5)
    m = B.Model(2, 5)
    m.upsert([4], [x[:2]])
    same_bits(m.feats(4), B.round_bf16(x[:2]))
    m.append([4, 9], [x[2:], x[:1]], keep="latest")
    same_bits(m.feats(4), B.round_bf16(x[1:]))
    same_bits(m.feats(9), B.round_bf16(x[:1]))


def test_cosine_f64_marks_absent_and_zero_rows():
    q = [np.array([[1.0, 0.0]], np.float32), np.zeros((0, 2), np.float32)]
    s = [np.array([[1.0, 0.0], [0.0, 0.0]], np.float32)]
    c = B.cosine_f64(q, s, 2)
    assert c.shape == (2, 2, 1, 2) and c[0, 0, 0, 0] == 1.0
    assert np.isnan(c[0, 0, 0, 1]) and np.isnan(c[0, 1]).all() and np.isnan(c[1]).all()
