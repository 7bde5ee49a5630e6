"""ThreadSanitizer run of the library's concurrency code (SURVEY.md §5 "race detection: TSan on the
CPU build").

tests/tsan builds csrc/tier1.cpp (key registry, per-thread lanes, the two-lane Tier-1
coalescing queue), csrc/multi.cpp (tfhe_gpu_init registry, per-device workers),
csrc/circuit.cpp (per-context device state) and the engine under them (csrc/engine.cpp,
csrc/host_batch.cpp) UNCHANGED with -fsanitize=thread; the stand-ins end at the kernel launchers
(tests/tsan/stub_kernels.cpp: deterministic hashes for the gate arithmetic) and the HIP host API
(tests/tsan/stub/).  Both drivers link the same objects.
The driver hammers them: 64 threads of Tier-1 gate chains with results aliasing inputs and mixed
gate kinds (the reference's OpenMP callers, cpuParallel/Cipher.cpp:83-120, cloud.cpp:389-395);
tfhe_gpu_boots_batch from 8 threads on either device while tfhe_gpu_init re-registers the key and
other keys are imported, registered, used and deleted; one circuit run concurrently on contexts
that come and go.  Every result is compared word for word (current_variance bit for bit) with
the same work done sequentially, and DeviceScope's save / restore logic is unit-tested with the
stub's per-thread current device.  Pass = exit 0 and no ThreadSanitizer report.

Round 5: the second driver (tests/tsan/_bin/tsan_engine) aims at
csrc/engine.cpp and csrc/host_batch.cpp (the host-pointer paths) themselves.  The stub HIP
runtime's streams are asynchronous worker threads, so a host read that is not ordered after
the stream work producing it is a race TSan sees.  tsan_engine_driver.cpp hammers the host copy
pool from three contexts (two devices, one a key replica built meanwhile), several threads on one
context at once, over the staged, sliced, record (LweSample rows + device current_variance) and
caller-owned pinned paths, plus the pinned registry under alloc / free churn; every result is
compared word for word with a sequential run.  A mutation check proves the harness can fail: the
same build with the pinned path's final stream synchronization deleted must draw a TSan report."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TSAN = os.path.join(HERE, "tsan")


def _run(exe, *args):
    cmd = [exe, *map(str, args)]
    # TSan maps its shadow memory at fixed addresses; without ASLR it never collides with a mapping
    if shutil.which("setarch"):
        cmd = ["setarch", os.uname().machine, "-R"] + cmd
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66 report_signal_unsafe=0")
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)


def _tsan_available():
    return shutil.which("g++") is not None and shutil.which("make") is not None


@pytest.mark.skipif(not _tsan_available(), reason="needs g++ and make")
def test_concurrency_code_is_tsan_clean():
    subprocess.run(["make", "-s", "-j4", "-C", TSAN], check=True, timeout=600)
    exe = os.path.join(TSAN, "_bin", "tsan_driver")
    cmd = [exe, "64", "8"]
    # TSan maps its shadow memory at fixed addresses; without ASLR it never collides with a mapping
    if shutil.which("setarch"):
        cmd = ["setarch", os.uname().machine, "-R"] + cmd
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66 report_signal_unsafe=0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    out = r.stdout + r.stderr
    assert "WARNING: ThreadSanitizer" not in out, out[-6000:]
    assert r.returncode == 0, out[-4000:]
    assert "tsan_driver: ok" in r.stdout
    for phase in ("tier1: 64 threads x 8 gates", "multi:", "circuits:"):
        assert phase in r.stdout, r.stdout


@pytest.mark.skipif(not _tsan_available(), reason="needs g++ and make")
def test_engine_host_side_is_tsan_clean():
    subprocess.run(["make", "-s", "-j4", "-C", TSAN, "_bin/tsan_engine"], check=True, timeout=600)
    r = _run(os.path.join(TSAN, "_bin", "tsan_engine"), 8, 2)
    out = r.stdout + r.stderr
    assert "WARNING: ThreadSanitizer" not in out, out[-6000:]
    assert r.returncode == 0, out[-4000:]
    assert "tsan_engine_driver: ok" in r.stdout
    for phase in ("sequential: 12 workloads", "engine host paths: 8 threads", "all equal", "pinned registry:"):
        assert phase in r.stdout, r.stdout


@pytest.mark.skipif(not _tsan_available(), reason="needs g++ and make")
def test_engine_tsan_harness_catches_a_missing_synchronization():
    """Mutation check: without the pinned host path's final wait for its streams (drain: the copy
    stream, then hipStreamSynchronize(c->stream)) the host reads results the (asynchronous) stub
    stream is still writing — the harness must report it."""
    src = open(os.path.join(HERE, "..", "cpu-gpu-tfhe_amd", "csrc", "host_batch.cpp")).read()
    cut = "    const hipError_t w = drain(c);\n    tr.lap(tr.wait);\n"
    assert src.count(cut) == 1, "the pinned path's final synchronization moved: update the mutation"
    os.makedirs(os.path.join(TSAN, "_bin"), exist_ok=True)
    mut = "// host_batch.cpp with the pinned path's final stream synchronization removed (mutation check)\n" + \
        src.replace(cut, "    const hipError_t w = hipSuccess;\n    tr.lap(tr.wait);\n")
    path = os.path.join(TSAN, "_bin", "host_batch_mut.cpp")
    if not os.path.exists(path) or open(path).read() != mut:
        open(path, "w").write(mut)
    subprocess.run(["make", "-s", "-j4", "-C", TSAN, "_bin/tsan_engine_mut"], check=True, timeout=600)
    r = _run(os.path.join(TSAN, "_bin", "tsan_engine_mut"), 4, 1)
    assert "WARNING: ThreadSanitizer" in r.stdout + r.stderr and r.returncode != 0
