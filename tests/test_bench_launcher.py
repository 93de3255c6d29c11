"""bench.py --gpus N must run on N ranks or refuse: the
launcher logic, on CPU, with a stubbed device count."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_launch_plan_decisions():
    import bench
    assert bench.launch_plan(1, {}, 1, []) == ('run', None)
    # a launcher with the right rank count: run
    assert bench.launch_plan(8, {'WORLD_SIZE': '8', 'LOCAL_RANK': '7'}, 8,
                             []) == ('run', None)
    # no launcher: re-execute as N ranks, arguments passed through
    action, cmd = bench.launch_plan(8, {}, 8, ['--gpus', '8', '--steps', '5'])
    assert action == 'spawn'
    assert '--nproc-per-node=8' in cmd and cmd[-4:] == ['--gpus', '8', '--steps', '5']
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    # refusals: a line that says n_gpus: N must have run on N GPUs
    with pytest.raises(SystemExit, match='only 1 GPU'):
        bench.launch_plan(8, {}, 1, [])
    with pytest.raises(SystemExit, match='only 1 GPU'):
        bench.launch_plan(8, {'WORLD_SIZE': '8'}, 1, [])
    with pytest.raises(SystemExit, match='WORLD_SIZE=2'):
        bench.launch_plan(8, {'WORLD_SIZE': '2'}, 8, [])
    with pytest.raises(SystemExit, match='WORLD_SIZE=2'):
        bench.launch_plan(1, {'WORLD_SIZE': '2'}, 8, [])
    with pytest.raises(SystemExit, match='no device'):
        bench.launch_plan(2, {'WORLD_SIZE': '2', 'LOCAL_RANK': '3'}, 2, [])


def test_bench_spawns_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher in the environment starts two
    ranks (torch.distributed.run on 127.0.0.1); with one visible device it
    exits non-zero and says why."""
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(LD_BENCH_FAKE_DEVICES='2', LD_BENCH_LAUNCH_ONLY='1')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2',
                        '--steps', '1', '--warmup', '0'], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout + r.stderr
    assert 'launch-only rank 0 of 2' in out and 'launch-only rank 1 of 2' in out
    env['LD_BENCH_FAKE_DEVICES'] = '1'
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2'],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert 'only 1 GPU' in r.stderr


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: one float64 file per loss key, and the same seeded sample
    of the parameter / gradient / momentum buffers (float32) from run to run."""
    import numpy as np
    import torch

    import bench
    from ld_amd.heads import LazyScalars

    class _Arena:
        flat_param = torch.arange(3 << 20, dtype=torch.float32)
        flat_grad = -flat_param

    class _Trainer:
        arena = _Arena()
        flat_momentum = _Arena.flat_param * 2

    out = dict(log_vars=LazyScalars(['loss_cls', 'loss'],
                                    torch.tensor([0.5, 1.25])))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), out, _Trainer())
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['grads_sample.npy', 'loss.npy', 'loss_cls.npy',
                     'momentum_sample.npy', 'params_sample.npy',
                     'sample_index.npy']
    total = 0
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / 'a' / 'loss.npy')) == 1.25
    idx = np.load(tmp_path / 'a' / 'sample_index.npy').astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'params_sample.npy'), idx)
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'momentum_sample.npy'),
                                  2 * idx)


def test_steps_must_be_positive(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '4',
                                      '--dump-outputs', 'out'])
    args = bench.parse()
    assert args.steps == 4 and args.dump_outputs == 'out'


def test_plain_run_times_the_headline_only(monkeypatch):
    """The legs beside the headline step run with --full only; the --no-*
    switches still turn single legs of a --full run off."""
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '4'])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--no-bf16'])
    args = bench.parse()
    assert args.full and args.no_bf16 and not args.no_graph
