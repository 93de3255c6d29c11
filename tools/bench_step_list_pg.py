"""The train step under a process group: eager enqueue against step lists replayed
in segments with the collectives issued in between (train.record_collectives,
ld_step_list_replay_until).  A 1-rank RCCL group with every collective forced
(LD_FORCE_COLLECTIVES=1) -- the only form one GPU admits -- at the bench
configuration: R50 <- R101, 2 x 800 x 1344, bf16 and fp32.

    python tools/bench_step_list_pg.py [--steps 30] [--warmup 8] [--timeout 420]
        [--precisions bf16,fp32] [--legs eager,graph_list,pipelined_list]
        [--label this_commit] [--out profiles/step_list_pg_latency.json]

Every (precision, leg) runs in a process of its own under its own time limit; the
first one that fails ends the run.  Per leg: the host time to enqueue one step on an
idle queue (median), the synchronised time per step of back-to-back steps, images/s,
and whether the leg is GPU-bound (it enqueues a step faster than the GPU runs one).
The result goes into the JSON under ``label`` (other labels in the file are kept: a
run of the eager leg on the parent commit is recorded next to this commit's)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ('eager', 'graph_list', 'pipelined_list')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def child(precision, leg, steps, warmup):
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.update(RANK='0', WORLD_SIZE='1', LD_FORCE_COLLECTIVES='1')
    sys.path.insert(0, REPO)
    import torch
    import torch.distributed as dist
    import ld_amd  # noqa: F401
    from ld_amd import layers as Y
    from ld_amd import model_zoo, synthetic
    from ld_amd import train as T
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    Y.set_precision(precision)
    det = model_zoo.build_seeded_ld_detector(50, 101, dev)
    tr = T.SGDTrainer(det, lr=model_zoo.OPTIMIZER['lr'])
    batches = []
    for g in (7, 5, 11):
        b = synthetic.synthetic_batch(2, (800, 1333), (800, 1344), g, 4321 + g)
        batches.append(dict(img=b['img'].to(dev), img_metas=b['img_metas'],
                            gt_bboxes=[x.to(dev) for x in b['gt_bboxes']],
                            gt_labels=[x.to(dev) for x in b['gt_labels']]))
    if leg == 'eager':
        st = T.AutoStepper(tr)
    else:
        st = T.AutoStepper(tr, mode=leg.split('_')[0], launcher='list')
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    dist.all_reduce = counted
    n = [0]

    def step():
        i = n[0]
        n[0] += 1
        return st.step(batches[i % 3], next_data=batches[(i + 1) % 3])

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    calls[0] = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    per_step_calls = calls[0] / steps
    # (now: a replayed step hands out the same static buffer every time)
    loss = float(out['log_vars']['loss'])
    idle = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        step()
        idle.append(time.perf_counter() - t1)
    torch.cuda.synchronize()
    idle.sort()
    host = idle[len(idle) // 2] * 1e3
    res = dict(precision=precision, leg=leg, steps=steps, warmup=warmup,
               mode=st.mode, launcher=st.launcher if st.mode != 'eager' else None,
               host_enqueue_ms=host, host_enqueue_ms_min=idle[0] * 1e3,
               back_to_back_issue_ms=t_issue / steps * 1e3,
               ms_per_step=dt / steps * 1e3, img_per_s=2 * steps / dt,
               all_reduce_per_step=per_step_calls, buckets=len(tr.arena.buckets),
               captures=st.captures, loss=loss)
    print('RESULT ' + json.dumps(res), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--timeout', type=int, default=420, help='seconds per leg')
    ap.add_argument('--precisions', default='bf16,fp32')
    ap.add_argument('--legs', default=','.join(LEGS))
    ap.add_argument('--label', default='this_commit')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles',
                                                  'step_list_pg_latency.json'))
    ap.add_argument('--child', nargs=2, metavar=('PRECISION', 'LEG'))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup)
    legs = a.legs.split(',')
    if any(leg not in LEGS for leg in legs):
        ap.error(f'legs are {LEGS}')
    results, failed = [], None
    for precision in a.precisions.split(','):
        for leg in legs:
            env = dict(os.environ, MASTER_ADDR='127.0.0.1',
                       MASTER_PORT=str(_free_port()))
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable,
                   os.path.abspath(__file__), '--steps', str(a.steps), '--warmup',
                   str(a.warmup), '--child', precision, leg]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
            if r.returncode != 0 or not line:
                failed = dict(precision=precision, leg=leg, returncode=r.returncode,
                              stderr=r.stderr[-2000:])
                print('FAILED', json.dumps(failed), flush=True)
                break  # nothing more on the GPU after a failure
            results.append(json.loads(line[-1][len('RESULT '):]))
            print(json.dumps(results[-1]), flush=True)
        if failed:
            break
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.setdefault('workload', 'LD R50 <- R101, 2 x 800x1344 (padded from 800x1333), '
                   'one MI355X, 1-rank RCCL group, LD_FORCE_COLLECTIVES=1')
    doc.setdefault('note', 'one rank on one GPU: nothing on more than one GPU was run')
    doc[a.label] = dict(results=results, failed=failed)
    # GPU time of a step: the fastest synchronised step any leg of that precision
    # reached (an eager leg's own step time may be its host time); a leg is
    # GPU-bound when it enqueues a step in less than that
    every = [r for v in doc.values() if isinstance(v, dict)
             for r in v.get('results', [])]
    for r in every:
        gpu = min(o['ms_per_step'] for o in every if o['precision'] == r['precision'])
        r['gpu_step_ms'] = gpu
        r['gpu_bound'] = bool(r['host_enqueue_ms'] < gpu)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
