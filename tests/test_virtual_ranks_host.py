"""CPU checks of virtual ranks (SGDTrainer(virtual_ranks=W), DESIGN.md section
6): the loader hands every step the W rank-local batches a W-process job would
load, the combinations this project does not run are refused by name, and the
arithmetic of ld_vrank_reduce (ld::vrank_mean, compiled for the host) is the
ascending-order fp32 sum followed by one division."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dataset_fixture as FX  # noqa: E402
import test_dataloader_host as TH  # noqa: E402  (TRAIN_PIPELINE, voc())

from ld_amd import dataloader as DL  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return FX.write_fixture(tmp_path_factory.mktemp('fixture'))


# ------------------------------------------------------------------ loader --
def _same_host(x, y):
    assert x['indices'] == y['indices']
    assert x['filenames'] == y['filenames']
    assert (x['epoch'], x['index']) == (y['epoch'], y['index'])
    assert repr(x['plans']) == repr(y['plans'])
    assert len(x['images']) == len(y['images'])
    for p, q in zip(x['images'], y['images']):
        np.testing.assert_array_equal(p, q)
    for k in ('gt_bboxes', 'gt_labels', 'gt_bboxes_ignore'):
        assert len(x[k]) == len(y[k])
        for p, q in zip(x[k], y[k]):
            assert p.dtype == q.dtype
            np.testing.assert_array_equal(p, q)


@pytest.mark.parametrize('W', (2, 4))
def test_loader_items_are_the_rank_loaders_batches(root, W):
    ds = TH.voc(root)
    vl = DL.build_dataloader(ds, 2, 1, seed=11, virtual_ranks=W)
    assert isinstance(vl, DL.VirtualRankLoader) and vl.virtual_ranks == W
    ranks = [DL.DeviceDataLoader(ds, 2, 1, dist=True, num_replicas=W, rank=r,
                                 seed=11) for r in range(W)]
    assert len(vl) == len(ranks[0]) > 0
    assert all(len(r) == len(vl) for r in ranks)
    for epoch in (0, 1):
        steps = list(vl.host_batches(epoch))
        assert len(steps) == len(vl)
        per_rank = [list(r.host_batches(epoch)) for r in ranks]
        for i, hosts in enumerate(steps):
            assert len(hosts) == W
            for r in range(W):
                _same_host(hosts[r], per_rank[r][i])
        # random access gives the same step
        for r, h in enumerate(vl.host_batch(epoch, len(vl) - 1)):
            _same_host(h, per_rank[r][-1])
    # the two epochs are ordered differently (the sampler is seeded per epoch)
    e0 = [h['indices'] for s in vl.host_batches(0) for h in s]
    e1 = [h['indices'] for s in vl.host_batches(1) for h in s]
    assert e0 != e1
    for r in ranks:
        r.close()
    vl.close()


def test_loader_one_pool_sized_by_workers_only(root):
    ds = TH.voc(root)
    for W in (2, 4):
        vl = DL.build_dataloader(ds, 2, 3, seed=1, virtual_ranks=W)
        assert vl.num_threads == DL.threads_for_workers(3) == 6
        list(vl.host_batches(0))
        pools = {id(r._pool) for r in vl.ranks}
        assert pools == {id(vl._pool)} and vl._pool._max_workers == 6
        vl.close()
        assert vl._pool is None and all(r._pool is None for r in vl.ranks)
    vl = DL.build_dataloader(ds, 2, 64, seed=1, virtual_ranks=8)
    assert vl.num_threads == 16
    vl.close()


def test_loader_look_ahead_is_bounded(root):
    """At most LOOK_AHEAD steps are started beyond the one handed out."""
    from ld_amd import datasets as D
    # all 8 images (the empty ones too): more steps than the look-ahead
    ds = D.VOCDataset(**dict(FX.dataset_kwargs(root)['voc_nofilter'][1],
                             pipeline=TH.TRAIN_PIPELINE))
    vl = DL.build_dataloader(ds, 1, 1, seed=3, virtual_ranks=2)
    started = []
    for r, ld in enumerate(vl.ranks):
        def _submit(order, epoch, index, _ld=ld, _r=r,
                    _orig=ld._submit):
            started.append((_r, index))
            return _orig(order, epoch, index)
        ld._submit = _submit
    n = len(vl)
    assert n > DL.LOOK_AHEAD + 1
    for k, _ in enumerate(vl.host_batches(0)):
        assert max(i for _, i in started) == min(k + DL.LOOK_AHEAD, n - 1)
    assert sorted(started) == [(r, i) for r in range(2) for i in range(n)]
    vl.close()


def test_loader_refusals(root):
    ds = TH.voc(root)
    with pytest.raises(NotImplementedError, match='virtual_ranks=0'):
        DL.build_dataloader(ds, 2, 1, virtual_ranks=0)
    with pytest.raises(NotImplementedError, match='dist=True'):
        DL.build_dataloader(ds, 2, 1, dist=True, virtual_ranks=2)
    with pytest.raises(NotImplementedError, match='test-mode'):
        DL.build_dataloader(TH.voc(root, train=False), 2, 1, virtual_ranks=2)


# ----------------------------------------------------------------- trainer --
def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))


def test_trainer_refuses_by_name(tmp_path):
    import torch.distributed as dist
    from ld_amd import train as T
    for W in (0, -2):
        with pytest.raises(NotImplementedError, match=f'virtual_ranks={W}'):
            T.SGDTrainer(_model(), lr=0.01, virtual_ranks=W)
    tr = T.SGDTrainer(_model(), lr=0.01, virtual_ranks=2)
    assert tr.virtual_ranks == 2 and tr._grad_scale() == 0.5
    assert T.SGDTrainer(_model(), lr=0.01).virtual_ranks == 1
    data = dict(img=torch.zeros(1, 3, 8, 8), img_metas=[{}])
    for launcher in ('graph', 'list'):
        with pytest.raises(NotImplementedError,
                           match=f"virtual_ranks=2 with GraphedStep.*{launcher}"):
            T.GraphedStep(tr, data, launcher=launcher)
        with pytest.raises(NotImplementedError,
                           match='virtual_ranks=2 with PipelinedGraphedStep'):
            T.PipelinedGraphedStep(tr, data, data, launcher=launcher)
        for mode in ('graph', 'pipelined'):
            with pytest.raises(NotImplementedError,
                               match=f"virtual_ranks=2 with AutoStepper.*{mode}"):
                T.AutoStepper(tr, mode=mode, launcher=launcher)
    assert T.AutoStepper(tr).mode == 'eager'  # the eager stepper is accepted
    # under a process group
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg',
                            rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError,
                           match='virtual_ranks=2 under a process group'):
            T.SGDTrainer(_model(), lr=0.01, virtual_ranks=2)
        T.SGDTrainer(_model(), lr=0.01, virtual_ranks=1)
    finally:
        dist.destroy_process_group()


def test_trainer_wrong_length_sequences():
    from ld_amd import train as T
    d = dict(img=torch.zeros(1, 3, 8, 8), img_metas=[{}])
    tr = T.SGDTrainer(_model(), lr=0.01, virtual_ranks=2)
    for bad in ([d], [d, d, d], [], d):
        with pytest.raises(ValueError, match='exactly 2'):
            tr.step(bad)
    assert tr.iter == 0
    one = T.SGDTrainer(_model(), lr=0.01)
    with pytest.raises(ValueError, match='1 rank'):
        one.step([d, d])


def test_from_config_takes_the_keyword():
    from ld_amd import train as T
    cfg = dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9,
                              weight_decay=0.0001),
               optimizer_config=dict(grad_clip=None))
    tr = T.SGDTrainer.from_config(_model(), cfg, virtual_ranks=8)
    # the config's lr is the W-rank job's: left as written
    assert tr.virtual_ranks == 8 and tr.lr == 0.01
    assert 'virtual_ranks' not in repr(tr.state_dict())


def test_epoch_runner_refuses_mismatched_ranks(root, tmp_path):
    from ld_amd import train as T
    from ld_amd.runner import EpochRunner
    vl = DL.build_dataloader(TH.voc(root), 2, 1, seed=1, virtual_ranks=2)
    tr = T.SGDTrainer(_model(), lr=0.01, virtual_ranks=4)
    cfg = dict(runner=dict(max_epochs=1))
    with pytest.raises(ValueError, match='2 virtual ranks.*trainer of 4'):
        EpochRunner(tr, cfg, tmp_path).run(vl)
    vl.close()


def test_train_tool_has_the_option():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        '_ld_train_tool', os.path.join(REPO, 'tools', 'train.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.parse_args(['cfg.py']).virtual_gpus == 1
    assert tool.parse_args(['cfg.py', '--virtual-gpus', '8']).virtual_gpus == 8


# ------------------------------------------------------------ reduce order --
@pytest.fixture(scope='module')
def hv():
    out_dir = os.path.join(REPO, 'tests', '_build')
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, 'libhost_harness_vrank.so')
    src = os.path.join(REPO, 'tests', 'host_harness_vrank.cpp')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off',
                           '-shared', '-fPIC', src, '-o', so])
    lib = C.CDLL(so)
    FP = C.POINTER(C.c_float)
    lib.h_vrank_reduce.argtypes = [FP, C.c_int, C.c_int, C.c_size_t, FP]
    lib.h_vrank_reduce.restype = None

    def reduce(table, stride=None):
        t = np.ascontiguousarray(table, dtype=np.float32)
        W, n = t.shape
        stride = n if stride is None else stride
        buf = np.zeros((W, stride), np.float32)
        buf[:, :n] = t
        out = np.full(n, np.nan, np.float32)
        lib.h_vrank_reduce(buf.ctypes.data_as(FP), W, n, stride,
                           out.ctypes.data_as(FP))
        return out
    return reduce


def _restated(table):
    """((p0 + p1) + ...) / W in float32."""
    t = np.asarray(table, np.float32)
    acc = t[0].copy()
    for r in range(1, t.shape[0]):
        acc = (acc + t[r]).astype(np.float32)
    return (acc / np.float32(t.shape[0])).astype(np.float32)


def test_reduce_is_the_ascending_sum_then_one_division(hv):
    # order matters: ascending gives ((1e8 + 1) - 1e8) + 1 = 0 + 1 -> 0.25;
    # the rows in descending order, or the pairwise (1e8 + 1) + (-1e8 + 1),
    # give 0; a float64 sum gives 0.5
    col = np.array([1e8, 1, -1e8, 1], np.float32)
    assert hv(col[:, None])[0] == np.float32(0.25)
    assert hv(col[::-1][:, None])[0] == np.float32(0.0)
    assert np.float64(col.astype(np.float64).sum()) / 4 == 0.5
    # divide AFTER the sum: 3 * (x / 3) and x rounded differently
    x = np.float32(0.1)
    t = np.array([[x], [x], [x]], np.float32)
    want = np.float32(np.float32(np.float32(x + x) + x) / np.float32(3))
    assert hv(t)[0] == want
    # a single rank is the identity
    assert hv(np.array([[3.5, -2.0]], np.float32)).tolist() == [3.5, -2.0]
    # every column on its own, any row stride
    rng = np.random.RandomState(5)
    for W in (2, 3, 4, 8):
        for n in (2, 9):
            t = (rng.randn(W, n) * 10.0 ** rng.randint(-3, 6, (W, n))) \
                .astype(np.float32)
            np.testing.assert_array_equal(hv(t), _restated(t))
            np.testing.assert_array_equal(hv(t, stride=n + 3), _restated(t))
