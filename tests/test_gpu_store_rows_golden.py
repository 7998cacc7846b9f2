"""Host-fed rows of a feature store on the MI355X against tests/golden/store_rows_parent.npz.

The fixture holds what upsert, append, a tapped search and fetch returned, fed from the host, when every store type still had a pad
kernel of its own for such rows (tests/golden/make_store_rows_golden.py; the commit is in the fixture's metadata).  A store now has
one fill path, k_pad_rows, for rows from anywhere, and the twin tests of test_gpu_devrows.py, test_gpu_i8.py, test_gpu_handover.py
and test_gpu_waste.py compare a device-fed call with "the host call's bits": this test says what those bits are.  No tolerance: every
recorded output is compared byte for byte (a large fetched row image by its SHA-256).  The cells of the tapped search carry the
norms of stored and query rows, the fetched rows the store's rounding.  The cases and why each width is there: store_rows_cases.py."""
import json
from pathlib import Path

import numpy as np
import pytest

import store_rows_cases as SC
from similari_amd import abi
from similari_amd.engine import Engine

FIXTURE = Path(__file__).resolve().parent / "golden" / "store_rows_parent.npz"


@pytest.fixture(scope="module")
def engine():
    eng = Engine(abi.make_config(device=0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_fixture_names_its_commit_and_every_case(golden):
    meta = json.loads(golden["meta"].tobytes().decode())
    assert len(meta["commit"]) == 40 and int(meta["commit"], 16) >= 0
    assert meta["cases"] == [SC.case_name(c) for c in SC.CASES] and meta["outputs"] == list(SC.OUTPUTS)
    assert sorted(golden) == sorted(["meta"] + [SC.case_name(c) + "/" + o for c in SC.CASES for o in SC.OUTPUTS])


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_name)
def test_host_fed_calls_return_the_recorded_bits(engine, golden, case):
    got = SC.recorded(SC.run_case(engine, case))
    for name in SC.OUTPUTS:
        want, have = golden[SC.case_name(case) + "/" + name], got[name]
        assert have.dtype == want.dtype and have.shape == want.shape, name
        assert have.tobytes() == want.tobytes(), "%s of %s differs from the recorded bits" % (name, SC.case_name(case))
