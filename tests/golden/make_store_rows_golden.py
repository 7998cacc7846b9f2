#!/usr/bin/env python
"""Records tests/golden/store_rows_parent.npz: what the host-fed calls of a feature store return and leave behind, bit for bit, for
the cases of tests/store_rows_cases.py.  Needs the MI355X and a built library; run by hand, not by pytest, at the commit whose bits
are to be pinned:

    python tests/golden/make_store_rows_golden.py --commit "$(git rev-parse HEAD)" [--out FILE]

The fixture was recorded at the last commit at which every store type had a pad kernel of its own for host-fed rows
(k_pad_features, k_pad_features_bf16, k_pad_features_f16, k_pad_features_i8), so it holds the bits of those kernels:
tests/test_gpu_store_rows_golden.py holds the one fill path that replaced them to it.  Record it again only if the stored bits are
meant to change.  The inputs are arithmetic (store_rows_cases.rows), so the file holds outputs and metadata only."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import store_rows_cases as SC  # noqa: E402
from similari_amd import abi  # noqa: E402
from similari_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit of the library that runs (kept in the fixture's metadata)")
    ap.add_argument("--out", default=str(HERE / "store_rows_parent.npz"))
    a = ap.parse_args()
    arrays = {}
    eng = Engine(abi.make_config(device=0))
    try:
        for case in SC.CASES:
            for name, v in SC.recorded(SC.run_case(eng, case)).items():
                arrays[SC.case_name(case) + "/" + name] = v
    finally:
        eng.close()
    meta = {"commit": a.commit, "device": "MI355X (gfx950)", "cases": [SC.case_name(c) for c in SC.CASES], "outputs": list(SC.OUTPUTS),
            "feats": "a row image above %d bytes is its SHA-256" % SC.FULL_BYTES}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(a.out, **arrays)
    print("%s: %d cases, %d bytes" % (a.out, len(SC.CASES), Path(a.out).stat().st_size))


if __name__ == "__main__":
    main()
