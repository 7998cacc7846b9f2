"""Child process of tests/test_gpu_points.py::test_points_of_a_torch_tensor_on_the_gpu — a process of its own because it needs torch's
HIP context (the stand-in for a pose network's output) next to the engine's, initialised first."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
torch.zeros(1, device="cuda:0")  # torch's context first, as in a process that runs its pose model before the tracker

from similari_amd import abi  # noqa: E402
from similari_amd.devrows import DeviceRows, register_tensor  # noqa: E402
from similari_amd.engine import Engine, EngineError  # noqa: E402
from similari_amd.points import SA_ROW_NONE, PointBank  # noqa: E402


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def main():
    g = torch.Generator().manual_seed(78)
    B, P, comps = 25, 17, 3
    L = P * comps
    W = L + 13
    ids = np.arange(1, 20, dtype=np.uint64)
    n = len(ids)
    index = np.array([24, 3, 3, SA_ROW_NONE, 0, 7, 8, 9, 10, 11, SA_ROW_NONE, 12, 13, 20, 21, 22, 23, 1, 2], np.uint32)
    got = index != SA_ROW_NONE
    eng = Engine(abi.make_config(device=0))
    try:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            dev, host = PointBank(eng, P), PointBank(eng, P)
            try:
                for k in range(3):
                    t = torch.randn(B, W, generator=g) * 40
                    t[:, 6 + 2: 6 + L: comps] = torch.rand(B, P, generator=g)   # the scores
                    t[7, 6] = float("nan")
                    t = t.to(dtype).to("cuda:0")   # the "pose output": L of its W columns are the keypoints
                    view = t[:, 6: 6 + L]          # a column slice: row stride W
                    wide = view.float().cpu().numpy().reshape(B, P, comps)   # widen, exactly
                    torch.cuda.synchronize()       # the rows are final before the bank reads them
                    z = np.zeros((n, P, comps), np.float32)
                    z[got] = wide[index[got]]
                    mask = np.repeat(got[:, None], P, 1)
                    rows = DeviceRows.from_tensor(view, index)
                    assert (rows.ptr, rows.n_rows, rows.row_stride) == (t.data_ptr() + 6 * t.element_size(), B, W)
                    try:
                        dev.step(ids, rows=rows, comps=comps, min_score=0.3)
                        raise AssertionError("an unregistered tensor was accepted")
                    except EngineError as err:
                        assert err.code == abi.SA_ERR_BAD_ARG and "registered" in str(err)
                    with register_tensor(eng, t):
                        xy = dev.step(ids, rows=rows, comps=comps, min_score=0.3)
                        st = dev.last()
                        assert bits(xy, host.step(ids, z, present=mask, min_score=0.3)), (dtype, k)
                        assert st["launches"] == 1 and st["bytes_h2d"] == 2 * n * 4
                        assert st["src_bytes"] == int(got.sum()) * L * t.element_size()
                        for mode in ("d2", "cost", "cost_inverted"):
                            assert bits(dev.distance(ids, rows=rows, comps=comps, min_score=0.3, mode=mode),
                                        host.distance(ids, z, present=mask, min_score=0.3, mode=mode)), (dtype, mode)
                        try:   # a span that runs past the tensor's storage
                            dev.step(ids, rows=DeviceRows(rows.ptr, B + 1, W, rows.elem, index), comps=comps)
                            raise AssertionError("a span past its block was accepted")
                        except EngineError as err:
                            assert err.code == abi.SA_ERR_BAD_ARG
                for i in ids:
                    x, y = dev.state(i), host.state(i)
                    assert (x[0] == y[0]).all() and bits(x[1], y[1]) and bits(x[2], y[2]), i
                assert dev.state(1)[0].any() and not dev.state(4)[0].any() and np.isnan(xy[3]).all()
            finally:
                dev.close()
                host.close()
    finally:
        eng.close()
    print("POINT-ROWS-OK")


if __name__ == "__main__":
    main()
