"""Child process of tests/test_gpu_devrows.py::test_rows_of_a_torch_tensor_on_the_gpu — a process of its own because it needs torch's
HIP context (the stand-in for a ReID model's output) next to the engine's, initialised first."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
torch.zeros(1, device="cuda:0")  # torch's context first, as in a process that runs its ReID model before the tracker

from similari_amd import abi  # noqa: E402
from similari_amd.devrows import DeviceRows, DeviceRowsStore, register_tensor  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402
from similari_amd.f16 import SA_ELEM_BF16, SA_ELEM_F16, SA_ELEM_F32  # noqa: E402


def bits(*arrays):
    return [None if a is None else np.ascontiguousarray(a).tobytes() for a in arrays]


def main():
    g = torch.Generator().manual_seed(77)
    B, W, D, K = 40, 48, 33, 3
    ids = np.arange(1, 11, dtype=np.uint64)
    n_obs = np.array([3, 0, 2, 3, 1, 3, 2, 3, 3, 1], np.uint32)              # 21 rows of the 40
    q_ids = np.arange(100, 104, dtype=np.uint64)
    q_n_obs = np.array([2, 3, 0, 3], np.uint32)
    q_index = np.array([39, 38, 30, 31, 31, 5, 22, 23], np.uint32)           # gathered; a row named twice, a stored row among them
    eng = Engine(abi.make_config(device=0))
    try:
        for dtype, store_elem, kind in ((torch.float16, SA_ELEM_F16, "euclidean"), (torch.bfloat16, SA_ELEM_F32, "cosine"),
                                        (torch.float16, SA_ELEM_BF16, "cosine")):
            t = (torch.randn(B, W, generator=g) * 4).to(dtype).to("cuda:0")  # the "ReID output": D of its W columns are the embedding
            view = t[:, 4:4 + D]                                             # a column slice: row stride W, base 4 elements in
            host = view.float().cpu().numpy()                                # widen, exactly
            torch.cuda.synchronize()                                         # the rows are final before the store reads them
            a, b = DeviceRowsStore(eng, kind, D, K, store_elem), DeviceRowsStore(eng, kind, D, K, store_elem)
            try:
                with register_tensor(eng, t):
                    rows = DeviceRows.from_tensor(view)
                    assert (rows.ptr, rows.n_rows, rows.row_stride) == (t.data_ptr() + 4 * t.element_size(), B, W)
                    a.upsert_rows(ids, n_obs, rows)
                    assert a.devrows_stats()["rows"] == int(n_obs.sum())
                    off = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int64)
                    b.upsert(ids, [host[off[i]:off[i + 1]] for i in range(len(ids))])
                    assert bits(*a.fetch_raw(ids)) == bits(*b.fetch_raw(ids))
                    q_rows = DeviceRows.from_tensor(view, q_index)
                    qo = np.concatenate([[0], np.cumsum(q_n_obs)]).astype(np.int64)
                    q_host = [host[q_index[qo[i]:qo[i + 1]]] for i in range(len(q_ids))]
                    got = a.search_rows_raw(q_ids, q_n_obs, q_rows, 3, 3.0e38, tap=True)
                    assert bits(*got) == bits(*b.search_raw(q_ids, q_host, 3, 3.0e38, tap=True))
                    assert got[0].sum() > 0
                    assert a.search_rows(q_ids, q_n_obs, q_rows, 2, 3.0e38, vote="bestfit") == b.search_bestfit(q_ids, q_host, 2, 3.0e38)
            finally:
                a.close()
                b.close()
    finally:
        eng.close()
    print("DEVICE-ROWS-OK")


if __name__ == "__main__":
    main()
