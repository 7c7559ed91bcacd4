"""bench.py without --full runs the headline only, and --dump-outputs writes
what the last timed step left for its caller.

A run without --full sets up, warms up, times exactly --steps steps and prints
its line: no verification, CPU baseline, host path, shape legs, decode legs or
probes (their fields are null). --dump-outputs DIR writes a fixed sample of
the records of the chunks the output slots still hold after the last timed
step; here every file is compared with the CPU oracle's encoding and decoding
of the same records, at positions worked out in numpy from the documented
sample (bench.dump_sample, bench.sample_bytes), and two runs with the same
arguments write the same files."""
import json
import os

import numpy as np
import pytest

import bench
from honu_amd.metadata import HostBatch
from honu_amd.workload import gen_host_batch

torch = pytest.importorskip("torch")


def test_headline_only_switches():
    """Argument handling only (no GPU): --full is off by default and a run
    without it drops every extra leg and check; with it nothing changes."""
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    assert bench.legs_of(a) == ["small", "mixed_encode", "medium", "xlarge"]
    bench.headline_only(a)
    assert a.no_cpu_baseline and a.no_verify and a.no_host_path and a.no_decode_legs
    assert bench.legs_of(a) == [] and a.decode_leg == "materialising"
    f = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert f.full is True and f.dump_outputs == "d"
    assert not (f.no_cpu_baseline or f.no_verify or f.no_host_path or f.no_decode_legs)
    z = bench.parse_args(["--decode-leg", "zero_copy"])
    bench.headline_only(z)
    assert z.decode_leg == "zero_copy"  # an explicit leg stays


def _expected_bytes(arena, start, length, frac):
    """sample_bytes as its docstring states it, in numpy, one range at a time."""
    q = bench.DUMP_BYTES // 4
    out = np.full((len(start), bench.DUMP_BYTES), -1.0, np.float32)
    for r, (s, ln) in enumerate(zip(start, length)):
        s, ln = int(s), int(ln)
        if ln <= 0:
            continue
        head = [j % ln for j in range(q)]
        mid = [min(int(f * float(ln)), ln - 1) for f in frac]
        tail = [max(ln - q + j, 0) % ln for j in range(q)]
        out[r] = arena[s + np.array(head + mid + tail, np.int64)]
    return out


def _line(capsys):
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n", [("mixed", 1500), ("small", 9000)])
def test_plain_run_dumps_last_step(oracle_lib, tmp_path, capsys, shape, n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    seed, steps, chunks = 13, 3, 3
    argv = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--records", str(n), "--shape", shape,
            "--min-chunks", str(chunks), "--seed", str(seed)]
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.main(argv + ["--dump-outputs", d1])
    out = _line(capsys)
    # the headline's fields, and nothing beside it
    assert out["full"] is False and out["steps"] == steps and out["ms_per_step"] > 0
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    gib = out["config"]["encoded_bytes_per_gpu"] / 2**30
    assert abs(out["value"] - gib / (out["ms_per_step"] / 1e3)) <= 1e-9 * out["value"]
    assert out["roofline"]["launches"] == steps * out["config"]["chunks"]  # --steps steps were timed
    for k in ("verified", "decode", "legs", "host_path", "scatter"):
        assert out[k] is None, k
    assert "cpu_baseline" not in out and out["kernels"]["hbm_probe"] is None
    assert out["kernels"]["zero_copy_decode_records_per_s"] is None

    files = _load(d1)
    assert all(v.dtype in (np.float32, np.float64) and v.size for v in files.values())
    assert sum(v.nbytes for v in files.values()) <= 64 << 20
    # the same arguments, the same files
    bench.main(argv + ["--dump-outputs", d2])
    _line(capsys)
    again = _load(d2)
    assert files.keys() == again.keys()
    for k in files:
        assert files[k].tobytes() == again[k].tobytes(), k

    # two slots: the step's last two chunks are still there
    b = bench.Bench(bench.parse_args(argv), 0, 0)
    held = b.chunks[-2:]
    b.release()
    assert len(b.chunks) == chunks
    assert {k.split("_")[0] for k in files} == {f"chunk{a}" for a, _ in held}
    hb = gen_host_batch(seed, shape, 0, n)
    for a, z in held:
        g = lambda name: files[f"chunk{a}_{name}"]  # noqa: E731
        idx, frac = bench.dump_sample(z - a, bench.DUMP_RECORDS // 2)
        assert len(idx) == min(z - a, bench.DUMP_RECORDS // 2) and len(set(idx)) == len(idx)
        sub = HostBatch(hb.meta[a:z], hb.var, hb.acl, hb.regions, hb.payload, hb.payload_off[a:z + 1])
        oout, ooff, ost = oracle_lib.marshal_batch(sub)
        ooff = ooff.astype(np.int64)
        assert np.array_equal(g("records"), (idx + a).astype(np.float64))
        assert np.array_equal(g("out_off"), np.stack([ooff[idx], ooff[idx + 1]], 1).astype(np.float64))
        assert np.array_equal(g("status"), ost[idx].astype(np.float32))
        assert np.array_equal(g("encoded"), _expected_bytes(oout, ooff[idx], ooff[idx + 1] - ooff[idx], frac))
        ometa, oinfo, oacl, oreg, odata, otot = oracle_lib.decode_batch(oout, ooff.astype(np.uint64), True)
        rows = ometa.view(np.uint8).reshape(z - a, 352)
        info = oinfo.view(np.uint8).reshape(z - a, 32)
        assert np.array_equal(g("rows"), rows[idx].astype(np.float32))
        assert np.array_equal(g("info"), info[idx].astype(np.float32))
        doff = oinfo["data_off"].astype(np.int64)[idx]
        dlen = oinfo["data_len"].astype(np.int64)[idx]
        assert np.array_equal(g("data"), _expected_bytes(odata, doff, dlen, frac))
        assert np.array_equal(g("totals"), otot.astype(np.float64))
        # the tables: a fixed shape, -1 past the last entry
        for what, tab, width in (("acl_table", oacl, 20), ("region_table", oreg, 4)):
            want = np.full((bench.DUMP_TABLE, width), -1.0, np.float32)
            ent = np.ascontiguousarray(tab).view(np.uint8).reshape(-1, width)[: bench.DUMP_TABLE]
            want[: len(ent)] = ent
            assert np.array_equal(g(what), want), what
