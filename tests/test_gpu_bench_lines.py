"""bench.py's BASELINE config-3 lines on a small batch, on the GPU: the Get
as Client.decode runs it (client/ecRedis.go:404-427), fused (dec4_get) and
unfused (dec4_upstream).  Each line names the kernel the library runs
(gf_apply_tri for these shapes), proves its work (garbage into the rebuilt
rows, bit-exact compare) and its checks (one corrupted byte of an extra
parity shard flags exactly its object), and carries a CPU leg that runs the
Go path's Reconstruct + Verify, bit-exact against the GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(workload, *more):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--batch", "16",
           "--steps", "2", "--warmup", "1", *more]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("workload,kernel", [("dec4_get", "gf_apply_tri<12,4>"),
                                             ("dec4_upstream", "gf_apply_tri<14,4>")])
def test_config3_get_lines(gpu, workload, kernel):
    out = _line(workload, "--cpu-seconds", "1", "--no-pmc", "--full")
    assert out["config"]["k"] == 10 and out["config"]["p"] == 4 and out["config"]["batch_per_gpu"] == 16
    r = out["roofline"]
    assert r["kernel"].startswith(kernel) and 0 < r["frac"] < 1
    wc = out["work_check"]["decode"]
    assert wc["result"] == "bit-exact" and wc["rows_rewritten"] == 32
    assert wc["corruption_check"]["flagged"] == [8] and wc["corruption_check"]["row"] == 13
    cpu = out["cpu_baseline"]
    assert "Reconstruct then Verify" in cpu["decode_form"] and cpu["sample"].endswith(": True")
    if workload == "dec4_get":
        assert cpu["fused_form_GiBps"] > 0
        # 12 rows read + 2 written per object
        assert r["kernel"].split("), ")[1].startswith(str(16 * 14 * ((4 << 20) // 10 + 1)))
    else:
        assert set(r["kernel_ms_alone"]) == {"decode:reconstruct", "decode:verify"}


def test_plain_run_headline_fields_and_dumped_outputs(gpu, tmp_path):
    """A run without --full prints the headline fields alone and, with
    --dump-outputs, writes the last timed step's written rows (a fixed sample)
    and decode flags as float32; a second run with the same arguments writes
    the same arrays."""
    import numpy as np
    outs = []
    for d in ("a", "b"):
        out = _line("encdec", "--dump-outputs", str(tmp_path / d))
        assert out["unit"] == "GiB/s" and out["dtype"] == "u8" and out["higher_is_better"] is True
        assert out["steps"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
        assert out["config"]["batch_per_gpu"] == 16
        for moved in ("roofline", "work_check", "cpu_baseline", "strong_scaling"):
            assert moved not in out
        assert sorted(os.listdir(tmp_path / d)) == ["decode_flags.npy", "rows_written.npy"]
        outs.append({f: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)})
    rows, flags = outs[0]["rows_written.npy"], outs[0]["decode_flags.npy"]
    S = ((1 << 20) + 9) // 10
    # 16 objects x (data rows 0, 5 + parity rows 10, 11) x every column (fits the sample)
    assert rows.dtype == np.float32 and rows.shape == (16, 4, S)
    assert flags.dtype == np.float32 and flags.shape == (16,) and not flags.any()
    assert rows.min() >= 0 and rows.max() <= 255 and np.array_equal(rows, np.rint(rows))
    assert len(np.unique(rows[:, 2:])) == 256  # parity rows hold coded bytes, not zeros
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f]), f


def test_dumped_rows_of_a_mixed_batch_are_a_valid_code(gpu, tmp_path):
    """Where every object lost its own pair of shards the dump holds all 12
    rows of each sampled column: after the last step's encode and decode the
    parity rows are the oracle's encode of the data rows, byte for byte."""
    import numpy as np

    import oracle
    from oracle import rs_numpy as rn
    out = _line("encdec_mixed", "--dump-outputs", str(tmp_path))
    assert out["value"] > 0
    rows = np.load(tmp_path / "rows_written.npy")
    assert rows.dtype == np.float32 and rows.shape == (16, 12, 65536)  # 12 Mi bytes over 16 x 12 rows
    assert not np.load(tmp_path / "decode_flags.npy").any()
    b = rows.astype(np.uint8)
    assert np.array_equal(b, rows) and len(np.unique(b[:, :10])) == 256
    m = rn.build_matrix(10, 2)
    for o in range(16):
        want = oracle.apply(m[10:], [b[o, c] for c in range(10)])
        for r in range(2):
            assert np.array_equal(b[o, 10 + r], want[r]), (o, r)
