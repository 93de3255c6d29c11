"""Step lists under a process group, the host side on CPU (2 gloo ranks): the
recording state of the collectives (``record_collectives``), the plan it fills
(``CollectivePlan``) and the driver that issues the plan's collectives between the
segments of a replay (``CollectivePlan.run``, what ``_StepList.replay_segments``
calls).  The list is a fake: a script of nodes (closures that do the captured
arithmetic and log themselves) and cut marks.

The contract pinned here: a rank that replays issues the collectives of a rank that
steps eagerly at the same iteration, in the same order -- normaliser, logs, buckets
in bucket order -- and each one after everything enqueued before its mark and
before everything after it."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _FakeList:
    """``script``: ('node', name, fn) entries are enqueued (run and logged) in
    order; ('mark', i) hands control to the driver, as ld_step_list_replay_until
    does at a cut mark."""

    def __init__(self, script, log):
        self.script, self.log = script, log

    def segments(self, device=None):
        for item in self.script:
            if item[0] == 'node':
                item[2]()
                self.log.append(('node', item[1]))
            else:
                yield item[1], None


class _LoggedWork:
    def __init__(self, work, log, tag):
        self.work, self.log, self.tag = work, log, tag

    def wait(self):
        self.log.append(('wait', self.tag))
        return self.work.wait()


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(),
                               torch.nn.Linear(32, 8), torch.nn.Linear(8, 4))


def _backward(model, arena, rank):
    torch.manual_seed(1)
    x, y = torch.randn(8, 16), torch.randn(8, 4)
    sl = slice(rank * 4, rank * 4 + 4)
    arena.zero_grad()
    ((model(x[sl]) - y[sl])**2).sum(1).mean().backward()


def _plan_worker(rank, world, port, ret):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from ld_amd import train as T
        from ld_amd.heads import GFLHead
        model = _model()
        arena = T.GradArena(list(model.parameters()), bucket_bytes=600)
        nb = len(arena.buckets)
        assert nb == 3, nb
        ws = float(world)
        norm_local = torch.tensor([3.0 + rank, 1.5 * (rank + 1)])
        logs_local = torch.tensor([1.0 + rank, 2.0 * rank, 4.0])
        norm, logged = torch.zeros(2), torch.zeros(3)
        log = []
        if rank == 0:
            # the eager way, through the real sites
            norm.copy_(norm_local)
            GFLHead._norm_reducer()(norm)
            logged.copy_(logs_local)
            dist.all_reduce(logged.div_(ws))
            _backward(model, arena, rank)
            arena.finish()
        else:
            real = dist.all_reduce
            n_calls = [0]

            def logged_all_reduce(t, *a, **k):
                n_calls[0] += 1
                log.append(('all_reduce', n_calls[0] - 1))
                w = real(t, *a, **k)
                return _LoggedWork(w, log, n_calls[0] - 1) if k.get('async_op') \
                    else w

            dist.all_reduce = logged_all_reduce
            try:
                plan = T.CollectivePlan()
                # what a capture records: the two synchronous marks by hand (their
                # arithmetic lives in the fake list's nodes), the buckets through
                # the arena's own issue / wait sites
                assert plan.add('sync', norm) == 0
                assert plan.add('sync', logged) == 1
                with T.record_collectives(plan):
                    _backward(model, arena, rank)
                    arena.finish()
                assert n_calls[0] == 0  # nothing was issued while recording
                kinds = [k for k, _, _ in plan.entries]
                assert kinds == ['sync', 'sync'] + ['issue'] * nb + ['wait'] * nb
                assert [r for _, _, r in plan.entries[2 + nb:]] == [2, 3, 4]
                assert plan.collectives == nb + 2 and len(plan) == 2 * nb + 2
                for (k, t, _), bk in zip(plan.entries[2:2 + nb], arena.buckets):
                    assert t.data_ptr() == arena.flat_grad.data_ptr() + 4 * bk['start']
                    assert t.numel() == bk['end'] - bk['start']
                script = [
                    ('node', 'norm_partials', lambda: norm.copy_(norm_local)),
                    ('mark', 0),
                    ('node', 'norm_div', lambda: norm.div_(ws)),
                    ('node', 'logs_div', lambda: logged.copy_(logs_local).div_(ws)),
                    ('mark', 1),
                    ('node', 'backward_a', lambda: None),
                    ('mark', 2),                       # issue bucket 0
                    ('node', 'backward_b', lambda: None),
                    ('mark', 3),                       # issue bucket 1
                    ('node', 'backward_c', lambda: None),
                    ('mark', 4),                       # issue bucket 2
                    ('node', 'join', lambda: None),
                    ('mark', 5),                       # wait bucket 0: after 2 later issues
                    ('mark', 6),
                    ('mark', 7),
                    ('node', 'sgd', lambda: None),
                ]
                plan.run(_FakeList(script, log).segments())
            finally:
                dist.all_reduce = real
            assert n_calls[0] == nb + 2
            assert log == [
                ('node', 'norm_partials'), ('all_reduce', 0), ('node', 'norm_div'),
                ('node', 'logs_div'), ('all_reduce', 1), ('node', 'backward_a'),
                ('all_reduce', 2), ('node', 'backward_b'), ('all_reduce', 3),
                ('node', 'backward_c'), ('all_reduce', 4), ('node', 'join'),
                ('wait', 2), ('wait', 3), ('wait', 4), ('node', 'sgd')], log
        # both ranks hold the same reduced values: the eager one's
        assert torch.allclose(norm, torch.tensor([3.5, 2.25]))
        assert torch.allclose(logged, torch.tensor([1.5, 1.0, 4.0]))
        state = torch.cat([norm, logged, arena.flat_grad])
        got = [torch.empty_like(state) for _ in range(world)]
        dist.all_gather(got, state)
        assert torch.equal(got[0], got[1])
        # the sums are those of the two ranks' local gradients
        local = _model()
        la = T.GradArena(list(local.parameters()), bucket_bytes=600)
        total = torch.zeros_like(la.flat_grad)
        with T.suspend_collectives():
            for r in range(world):
                _backward(local, la, r)
                la.finish()
                total += la.flat_grad
        assert torch.allclose(arena.flat_grad, total, rtol=1e-6, atol=1e-7)

        # a list with more marks than the plan has entries / fewer: both raise
        # (every rank runs the same thing, so the one all-reduce has its partner)
        def one_entry_plan():
            p = T.CollectivePlan()
            p.add('sync', torch.ones(2))
            return p

        with pytest.raises(RuntimeError, match='cut mark 1'):
            one_entry_plan().run(_FakeList([('mark', 0), ('mark', 1)], []).segments())
        p2 = one_entry_plan()
        p2.add('sync', torch.ones(2))
        with pytest.raises(RuntimeError, match='ended after 1 cut marks'):
            p2.run(_FakeList([('mark', 0)], []).segments())
        with pytest.raises(RuntimeError, match='cut mark 1'):  # out of order
            p2.run(_FakeList([('mark', 1)], []).segments())
        p3 = T.CollectivePlan()
        p3.add('issue', torch.ones(2))
        with pytest.raises(RuntimeError, match='nobody waited'):
            p3.run(_FakeList([('mark', 0)], []).segments())
        with pytest.raises(ValueError):
            p3.add('wait', ref=3)
        ret[rank] = 'ok'
    finally:
        dist.destroy_process_group()


def _state_worker(rank, world, port, ret):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from ld_amd import train as T
        from ld_amd.detectors import SingleStageDetector
        from ld_amd.heads import GFLHead
        model = _model()
        arena = T.GradArena(list(model.parameters()), bucket_bytes=600)
        nb = len(arena.buckets)
        real = dist.all_reduce
        calls = [0]

        def counting(*a, **k):
            calls[0] += 1
            return real(*a, **k)

        losses = dict(loss_a=[torch.tensor(1.0 + rank), torch.tensor(2.0)],
                      acc=torch.tensor(10.0 * rank))
        dist.all_reduce = counting
        try:
            plan = T.CollectivePlan()
            assert T.collectives_on() and T.recording_plan() is None
            with T.record_collectives(plan) as got:
                assert got is plan and T.recording_plan() is plan
                assert T.collectives_on()
                red = GFLHead._norm_reducer()
                assert red is not None  # the multi-rank normaliser path
                norm = torch.tensor([3.0 + rank, 1.5, 0., 0.])
                red(norm)
                # the arithmetic around the collective still happens
                assert torch.equal(norm[:2], torch.tensor([3.0 + rank, 1.5]) / world)
                loss, lv = SingleStageDetector._parse_losses(None, losses)
                assert float(loss) == 3.0 + rank
                arena.trace, arena.exposed = [], []  # event timing: skipped
                _backward(model, arena, rank)
                arena.finish()
                assert arena.trace == [] and arena.exposed == []
                arena.trace = arena.exposed = None
                assert arena._works == []
                n = len(plan)
                assert n == 2 + 2 * nb
                # suspension wins inside a recording
                with T.suspend_collectives():
                    assert not T.collectives_on()
                    assert T.recording_plan() is None
                    assert GFLHead._norm_reducer() is None
                    SingleStageDetector._parse_losses(None, losses)
                    _backward(model, arena, rank)
                    arena.finish()
                assert len(plan) == n and T.recording_plan() is plan
            assert T.recording_plan() is None and T.collectives_on()
            assert calls[0] == 0, calls  # no all-reduce while recording
            assert plan.entries[0][1] is norm and plan.entries[0][0] == 'sync'
            assert plan.entries[1][1] is lv._tensor
            # ... and a recording inside a suspension records nothing either
            with T.suspend_collectives():
                with T.record_collectives(T.CollectivePlan()) as inner:
                    assert not T.collectives_on()
                    _backward(model, arena, rank)
                    arena.finish()
                    assert len(inner) == 0
            assert calls[0] == 0
            # back to the plain state: the real collectives are issued
            _backward(model, arena, rank)
            arena.finish()
            assert calls[0] == nb
        finally:
            dist.all_reduce = real
        ret[rank] = 'ok'
    finally:
        dist.destroy_process_group()


def _spawn(worker):
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=worker, args=(r, world, port, ret))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0, 'worker failed'
    assert dict(ret) == {0: 'ok', 1: 'ok'}


def test_plan_driver_matches_an_eager_rank():
    """Rank 0 issues normaliser, logs and 3 bucket reductions eagerly, rank 1
    through a plan and a scripted list: same sums, and on rank 1 every collective
    sits between the nodes before and after its mark."""
    _spawn(_plan_worker)


def test_recording_state():
    """collectives_on() is True inside record_collectives, no dist.all_reduce is
    called while recording, suspend_collectives has priority in either nesting."""
    _spawn(_state_worker)
