"""bench.py's host-side rules that need no GPU: the slot default (a rank that holds an RCCL communicator runs fewer slots —
profiles/r02_dist_queues.txt), and what bench.py does on a machine without a GPU: it fails loudly (the engine has no CPU
path) and leaves NOTHING on stdout — stdout carries rank 0's one JSON line and nothing else, ever."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_slot_default_leaves_room_for_the_communicators_streams():
    import bench
    assert bench.default_slots(False) == 22
    assert bench.default_slots(True) == 18
    # the chip runs 24 queues of a process without time-slicing: alone the slots + the null stream stay under it by count,
    # beside a communicator the pool's cap does (torch's collective stream has a pool of its own: + 1)
    assert bench.default_slots(False) + 1 <= 24 and bench.queue_cap(22, False) == 23
    assert bench.queue_cap(bench.default_slots(True), True) == 20
    for s in range(1, 65):
        assert bench.queue_cap(s, True) + 1 <= 23          # at least one queue of margin whatever --streams says
        assert bench.queue_cap(s, False) <= 23
        assert bench.queue_cap(s, False) >= min(s + 1, 23)  # room for the slots + the null stream up to the limit


def test_bench_without_gpu_fails_loudly_and_prints_nothing_on_stdout():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a GPU is present: the contract test (-m gpu) covers stdout")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0
    assert r.stdout == "", r.stdout[-500:]
    assert "needs a GPU" in r.stderr


def test_dump_outputs_writes_float_arrays_and_samples_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import bench
    import zkemail_rs_amd  # noqa: F401
    from zkemail_rs_amd import _abi as A
    rec = np.zeros(100, dtype=A.RESULT_DTYPE)
    rec["status"] = np.arange(100)
    rec["body_hash"][:, 0] = np.arange(100) % 256
    arrays = bench.record_arrays(rec)
    assert "reserved" not in arrays and arrays["status"].dtype == np.float64 and arrays["body_hash"].dtype == np.float32
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    assert (np.load(tmp_path / "all" / "status.npy") == np.arange(100)).all()
    assert not (tmp_path / "all" / "sample_rows.npy").exists()
    # above the limit: the same seeded rows of every array, their indices beside them, from run to run
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", sum(a.nbytes for a in arrays.values()) // 4)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    rows = np.load(tmp_path / "s1" / "sample_rows.npy")
    assert 0 < len(rows) <= 25 and (rows == np.load(tmp_path / "s2" / "sample_rows.npy")).all()
    assert (np.load(tmp_path / "s1" / "status.npy") == rows).all()
    assert (np.load(tmp_path / "s1" / "body_hash.npy")[:, 0] == rows % 256).all()
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) < sum(a.nbytes for a in arrays.values())
