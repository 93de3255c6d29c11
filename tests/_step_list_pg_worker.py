"""Worker of tests/test_gpu_step_list_pg.py (own process: it owns a process
group).  An RCCL group of ONE rank with every collective forced
(LD_FORCE_COLLECTIVES=1), as in tests/_graph_pg_worker.py: the step-list steppers
capture under ``record_collectives`` and replay in segments, the host issuing the
real all-reduces between them.  Checked against plain ``SGDTrainer.step`` calls bit
for bit, all-reduce calls counted.  Prints one JSON line.

    python tests/_step_list_pg_worker.py bf16|fp32 graph|pipelined"""
import json
import os
import sys

os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
os.environ['RANK'] = '0'
os.environ['WORLD_SIZE'] = '1'
os.environ['LD_FORCE_COLLECTIVES'] = '1'
os.environ.pop('LD_GRAPH_COLLECTIVES', None)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import ld_amd  # noqa: E402,F401
from ld_amd import layers as Y  # noqa: E402
from ld_amd import model_zoo, synthetic  # noqa: E402
from ld_amd import train as T  # noqa: E402


def batch(seed, shape, gts, dev):
    b = synthetic.synthetic_batch(2, shape, shape, gts, seed)
    return dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                gt_labels=[x.to(dev) for x in b['gt_labels']])


def trainer(dev):
    det = model_zoo.build_seeded_ld_detector(18, 18, dev, loss_im_weight=2.0)
    return T.SGDTrainer(det, lr=0.01, bucket_bytes=4 << 20)


def main():
    precision = sys.argv[1] if len(sys.argv) > 1 else 'bf16'
    case = sys.argv[2] if len(sys.argv) > 2 else 'graph'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    Y.set_precision(precision)
    if case == 'graph':  # two padded shapes, changing GT counts
        seq = [batch(11, (128, 160), [3, 2], dev), batch(12, (128, 160), [1, 5], dev),
               batch(13, (160, 128), [2, 2], dev), batch(14, (128, 160), [4, 1], dev),
               batch(15, (160, 128), [6, 3], dev), batch(16, (128, 160), [2, 7], dev)]
    else:  # one shape throughout
        seq = [batch(11, (128, 160), [3, 2], dev), batch(12, (128, 160), [1, 5], dev),
               batch(14, (128, 160), [4, 1], dev), batch(16, (128, 160), [2, 7], dev)]
    calls = dict(all_reduce=0)
    real = dist.all_reduce

    def counted(*a, **k):
        calls['all_reduce'] += 1
        return real(*a, **k)

    dist.all_reduce = counted

    def run(make_stepper):
        tr = trainer(dev)
        stepper = make_stepper(tr)
        calls['all_reduce'] = 0  # the steps' collectives only
        losses = []
        for i, d in enumerate(seq):
            out = stepper(d, seq[min(i + 1, len(seq) - 1)])
            losses.append(float(out['log_vars']['loss']))
        torch.cuda.synchronize()
        return tr, losses, calls['all_reduce']

    res = dict(precision=precision, case=case, steps=len(seq),
               collectives_on=bool(T.collectives_on()), raised=None)
    tr0, l0, res['eager_all_reduce_calls'] = run(lambda tr: (lambda d, nxt: tr.step(d)))
    res['buckets'] = len(tr0.arena.buckets)
    auto = {}

    def make(tr):
        auto['s'] = T.AutoStepper(tr, mode=case, launcher='list')
        return lambda d, nxt: auto['s'].step(d, next_data=nxt)

    try:
        tr1, l1, res['list_all_reduce_calls'] = run(make)
    except Exception as e:  # the parent commit: the refusal
        res['raised'] = f'{type(e).__name__}: {e}'
        print(json.dumps(res), flush=True)
        dist.destroy_process_group()
        return
    st = auto['s']
    if case == 'graph':
        steps = list(st._graphs.values())
        lists, plans = [g.list for g in steps], [g.plan for g in steps]
    else:
        lists, plans = st._pipe.lists, st._pipe.plans
    res.update(
        captures=st.captures,
        params_equal=bool(torch.equal(tr0.arena.flat_param, tr1.arena.flat_param)),
        momentum_equal=bool(torch.equal(tr0.flat_momentum, tr1.flat_momentum)),
        losses_equal=l0 == l1, losses=l1,
        list_marks=[sl.info['marks'] for sl in lists],
        plan_collectives=[p.collectives for p in plans],
        plan_kinds=[''.join(k[0] for k, _, _ in p.entries) for p in plans],
        list_lanes=[sl.info['lanes'] for sl in lists])
    if case == 'graph':
        # a GraphedStep built directly under the group (its two warm-up steps are
        # real steps with collectives) + one replay = three eager steps
        d = seq[0]
        tr2 = trainer(dev)
        for _ in range(3):
            out_e = tr2.step(d)
        tr3 = trainer(dev)
        g = T.GraphedStep(tr3, d, warmup=2, launcher='list')
        g.copy_inputs(d)
        out_g = g.replay()
        torch.cuda.synchronize()
        res['direct_equal'] = bool(
            torch.equal(tr2.arena.flat_param, tr3.arena.flat_param) and
            torch.equal(tr2.flat_momentum, tr3.flat_momentum) and
            float(out_e['log_vars']['loss']) == float(out_g['log_vars']['loss']))
        res['direct_marks'] = g.list.info['marks']
        try:
            T.GraphedStep(tr3, d)
            res['default_launcher_refused'] = False
        except RuntimeError as e:
            res['default_launcher_refused'] = 'refused' in str(e)
    print(json.dumps(res), flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
