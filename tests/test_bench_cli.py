"""bench.py's command line: a plain run measures the headline only, --full adds the rest, --dump-outputs writes what the
timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not args.full and args.dump_outputs == "" and args.steps == 7 and args.warmup == 3
    args = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert args.full and args.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-1"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_outputs_float32_whole(tmp_path):
    logits = np.arange(6 * 12, dtype=np.float32).reshape(6, 12)
    labels = np.array([0, 3, 11, 2, 2, 7], dtype=np.int32)
    paths = bench.dump_outputs(str(tmp_path / "d"), {"logits": logits, "labels": labels})
    assert sorted(os.path.basename(p) for p in paths) == ["labels.npy", "logits.npy"]
    got_l, got_y = np.load(tmp_path / "d" / "logits.npy"), np.load(tmp_path / "d" / "labels.npy")
    assert got_l.dtype == np.float32 and got_y.dtype == np.float32
    assert np.array_equal(got_l, logits) and np.array_equal(got_y, labels.astype(np.float32))
    assert not (tmp_path / "d" / "rows.npy").exists()


def test_dump_outputs_samples_the_same_rows_within_the_limit(tmp_path):
    n = 1000
    feats = np.random.default_rng(1).standard_normal((n, 1, 99, 10)).astype(np.float32)
    ids = np.arange(n, dtype=np.int32)
    limit = 200 * (990 * 4 + 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"features": feats, "ids": ids}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= limit + 3 * 128  # + the .npy headers
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    r = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy"), r.astype(np.float32))  # the same rows of every array
    assert np.array_equal(np.load(tmp_path / "a" / "features.npy"), feats[r])
    for f in ("rows.npy", "ids.npy", "features.npy"):  # fixed sample: identical from run to run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_dump_outputs_names_ranks(tmp_path):
    bench.dump_outputs(str(tmp_path), {"logits": np.zeros((2, 12), np.float32)}, rank=1, world=2)
    assert os.listdir(tmp_path) == ["logits.rank1.npy"]


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run: exactly --steps timed steps, the headline fields, none of the --full extras, and the dumped logits /
    labels are the fused path's results for the seeded clips (checked against the CPU oracle on a few of them)."""
    import torch

    from oracle import dscnn as o_dscnn
    from oracle import psf_mfcc as o_mfcc

    B, out = 256, tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                           "--spinup", "5", "--batch", str(B), "--dump-outputs", str(out)],
                          env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, proc.stdout[-1000:]
    line = json.loads(lines[0])
    assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "clips/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-6)
    for extra in ("configs", "cpu_baseline", "parity_golden", "bf16_triple_same_context"):
        assert extra not in line
    assert sorted(os.listdir(out)) == ["labels.npy", "logits.npy"]
    logits, labels = np.load(out / "logits.npy"), np.load(out / "labels.npy")
    assert logits.dtype == np.float32 and logits.shape == (B, bench.NUM_CLASSES)
    assert labels.dtype == np.float32 and labels.shape == (B,)
    assert np.array_equal(labels, logits.argmax(axis=1).astype(np.float32))
    blob, _ = bench.bench_weights()
    state, off = {}, 0
    for k, shp in o_dscnn.state_shapes(bench.NUM_CLASSES).items():
        n = int(np.prod(shp))
        state[k] = torch.from_numpy(blob[off:off + n].reshape(shp).copy())
        off += n
    pick = [0, 1, 100, B - 1]
    clips = bench.synth_clips(B, seed=0)[pick]
    want = o_dscnn.forward(state, torch.from_numpy(o_mfcc.collate_pcm16(clips))).numpy()
    assert float(np.abs(logits[pick] - want).max()) <= 1e-4
