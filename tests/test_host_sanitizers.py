"""The host threading of the product under a thread and an address / undefined-behaviour sanitizer, without a GPU.

Three stand-alone programs (tests/host_san/*_main.cpp, each with its own main) are compiled with plain g++ and started as child
processes, the way tests/test_pool.py starts its program:

  pool     similari_amd/csrc/sa_pool.h       the fork-join pool
  cluster  similari_amd/csrc/sa_cluster.cpp  the router over one worker thread per shard
  tracker  similari_amd/csrc/sa_tracker.cpp  the facade: pool jobs, driver thread, result handles, device groups

The router and the facade run over tests/host_san/stub_engine.cpp, a test-only engine with host tables, the oracle's association and
sa_kalman.h as upkeep; the facade is held against the oracle's tracker after every request set.  A program passes when it exits 0,
prints its `ok` line (which carries its coverage counts) and the sanitizer printed no report.  Nothing is loaded into Python under a
sanitizer, no environment variable is set for the children, and nothing here needs a GPU.
"""
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SAN = ROOT / "tests" / "host_san"
CSRC = ROOT / "similari_amd" / "csrc"

BASE = ["g++", "-O1", "-g", "-std=c++17", "-pthread"]
SANITIZERS = {
    "thread": ["-fsanitize=thread"],
    "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}
# (rustc never contracts a*b+c: the units with the filter arithmetic — sa_kalman.h, the oracle — are built as oracle/Makefile builds them)
FP = ["-ffp-contract=off"]
STUB = [SAN / "stub_engine.cpp", ROOT / "oracle" / "oracle.cpp"]
PROGRAMS = {
    "pool": dict(sources=[SAN / "pool_main.cpp"], flags=["-I", str(CSRC)]),
    "cluster": dict(sources=[SAN / "cluster_main.cpp", CSRC / "sa_cluster.cpp", *STUB], flags=FP),
    # (tracker_main.cpp takes sa_tracker.cpp into its own translation unit: its coverage counters read the facade's state)
    "tracker": dict(sources=[SAN / "tracker_main.cpp", ROOT / "oracle" / "oracle_tracker.cpp", *STUB], flags=FP + ["-Wno-subobject-linkage"]),
}
REPORTS = ("WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "STUB ENGINE:")

PROBE = r"""
#include <cstdio>
#include <thread>
int main() { int v = 0; std::thread t([&] { v = 1; }); t.join(); printf("probe ok %d\n", v); return 0; }
"""
_probe = {}


def probe(sanitizer, tmp_factory):
    """Can a program built with this sanitizer be built and started here?  (None: yes; else the reason, with the output.)"""
    if sanitizer not in _probe:
        why = None
        if sys.platform != "linux" or not shutil.which("g++"):
            why = "needs linux and g++"
        else:
            d = tmp_factory.mktemp(f"probe_{sanitizer}")
            (d / "probe.cpp").write_text(PROBE)
            try:
                b = subprocess.run(BASE + SANITIZERS[sanitizer] + [str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True, timeout=300)
                if b.returncode != 0:
                    why = f"the {sanitizer} sanitizer probe does not build here:\n{b.stdout}{b.stderr}"
                else:
                    r = subprocess.run([str(d / "probe")], capture_output=True, text=True, timeout=120)
                    if r.returncode != 0 or not r.stdout.startswith("probe ok 1") or any(m in r.stderr for m in REPORTS):
                        why = f"the {sanitizer} sanitizer probe does not start cleanly here (exit {r.returncode}):\n{r.stdout}{r.stderr}"
            except (OSError, subprocess.TimeoutExpired) as ex:
                why = f"the {sanitizer} sanitizer probe: {ex}"
        _probe[sanitizer] = why
    return _probe[sanitizer]


def run_program(name, sanitizer, tmp_path, tmp_factory, timeout):
    why = probe(sanitizer, tmp_factory)
    if why:
        pytest.skip(why)
    # from here on a failure is a failure: the sanitizer works on this machine
    p = PROGRAMS[name]
    exe = tmp_path / f"{name}_{sanitizer}"
    cmd = BASE + SANITIZERS[sanitizer] + p["flags"] + [str(s) for s in p["sources"]] + ["-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, f"{' '.join(cmd)}\n{b.stdout}{b.stderr}"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{name} under the {sanitizer} sanitizer: exit {r.returncode}\n{out[-8000:]}"
    for marker in REPORTS:
        assert marker not in out, f"{name} under the {sanitizer} sanitizer: '{marker}'\n{out[-8000:]}"
    last = [ln for ln in r.stdout.splitlines() if ln.strip()][-1:]
    assert last and last[0].startswith("ok "), f"{name} under the {sanitizer} sanitizer printed no ok line\n{out[-8000:]}"
    print(f"{name} / {sanitizer}: {last[0]}")   # (pytest -s, or a failing test, shows the coverage counts)


@pytest.mark.parametrize("sanitizer", list(SANITIZERS))
def test_pool_under_sanitizer(sanitizer, tmp_path, tmp_path_factory):
    run_program("pool", sanitizer, tmp_path, tmp_path_factory, timeout=300)


@pytest.mark.parametrize("sanitizer", list(SANITIZERS))
def test_cluster_router_under_sanitizer(sanitizer, tmp_path, tmp_path_factory):
    run_program("cluster", sanitizer, tmp_path, tmp_path_factory, timeout=300)


@pytest.mark.parametrize("sanitizer", list(SANITIZERS))
def test_tracker_facade_under_sanitizer(sanitizer, tmp_path, tmp_path_factory):
    run_program("tracker", sanitizer, tmp_path, tmp_path_factory, timeout=900)


def test_stub_engine_defines_exactly_what_the_host_files_leave_undefined(tmp_path):
    """The stub's contract: the sa_* symbols sa_tracker.cpp and sa_cluster.cpp leave undefined in a host compile, no more and no fewer."""
    if sys.platform != "linux" or not shutil.which("g++") or not shutil.which("nm"):
        pytest.skip("needs linux, g++ and nm")

    def symbols(src, flag, extra=()):
        obj = tmp_path / (Path(src).stem + ".o")
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", *extra, "-c", str(src), "-o", str(obj)], check=True, timeout=600)
        out = subprocess.run(["nm", flag, str(obj)], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("sa_")}

    needed = symbols(CSRC / "sa_tracker.cpp", "-u") | symbols(CSRC / "sa_cluster.cpp", "-u")
    defined = symbols(SAN / "stub_engine.cpp", "--defined-only", FP)
    assert defined == needed, f"missing {sorted(needed - defined)}, not asked for {sorted(defined - needed)}"
