"""bench.py's contract: ``--steps`` sets the timed steps, the line carries ``ms_per_step``, a plain run measures the headline only
(everything else is behind ``--full``), and ``--dump-outputs DIR`` writes what the last timed step returned as DIR/<name>.npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT

DUMP_LIMIT = 64 * 2 ** 20


def test_plain_run_is_the_default():
    a = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(['--full', '--dump-outputs', 'd'])
    assert a.full and a.dump_outputs == 'd'


def test_write_outputs_keeps_dtypes_and_samples_large_outputs_the_same_way(tmp_path):
    big = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32).reshape(3, 1, -1)
    arrays = {'big': big, 'pose': torch.randn(16, 7, dtype=torch.float64), 'mask': torch.tensor([[True, False]])}
    for d in ('a', 'b'):
        bench.write_outputs(str(tmp_path / d), arrays)
    out = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in arrays}
    assert out['pose'].dtype == np.float64 and np.array_equal(out['pose'], arrays['pose'].numpy())
    assert out['mask'].dtype == np.float32 and out['mask'].tolist() == [[1.0, 0.0]]
    s = out['big']
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(s) > 0) and s[-1] < big.numel()          # sorted, distinct elements of the output itself
    for n in arrays:
        assert np.array_equal(np.load(tmp_path / 'b' / f'{n}.npy'), out[n])


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_step(tmp_path):
    d = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--dump-outputs', str(d)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 2 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(16 * 1e3 / line['ms_per_step'], rel=1e-9)
    for k in ('metric', 'unit', 'higher_is_better', 'dtype'):
        assert k in line
    for k in ('roofline', 'cpu_baseline', 'value_conv_bf16x3', 'tracker_fps', 'latency_batch1_ms'):
        assert k not in line, k                                      # --full only
    files = sorted(os.listdir(d))
    assert files == sorted(f'{n}.npy' for n in ('pose', 'depth1', 'depth2', 'w2d', 'w3d', 'time_flow', 'stereo_flow2', 'mask2'))
    assert sum(os.path.getsize(d / f) for f in files) <= DUMP_LIMIT
    for f in files:
        x = np.load(d / f)
        assert x.dtype in (np.float32, np.float64) and x.size > 0, f
    pose = np.load(d / 'pose.npy')
    assert pose.shape == (16, 7) and np.isfinite(pose).all()
