"""Step lists under a process group (-m gpu): the captured step is cut where its
collectives belong and replayed segment by segment, the host issuing the real
``dist.all_reduce`` calls in between (train.record_collectives / CollectivePlan,
ld_step_list_replay_until).  No RCCL call is made while a stream captures, so the
race with ProcessGroupNCCL's watchdog that makes ``launcher='graph'`` refuse cannot
occur.  One-rank RCCL group with the collectives forced -- the only form one GPU
admits; the worker is tests/_step_list_pg_worker.py."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(precision, case):
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable,
                        os.path.join(REPO, 'tests', '_step_list_pg_worker.py'),
                        precision, case], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    print(res)
    return res


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_auto_stepper_list_under_process_group(precision):
    res = _run(precision, 'graph')
    assert res['collectives_on']
    # AutoStepper(tr, mode='graph', launcher='list') captures and replays under the
    # group (before cut marks existed: the RuntimeError of
    # _refuse_collectives_in_capture)
    assert res['raised'] is None, res['raised']
    assert res['params_equal'] and res['momentum_equal'] and res['losses_equal'], res
    nb = res['buckets']
    assert nb >= 2
    # 6 steps x (buckets + normaliser + logs), eager and replayed alike
    assert res['eager_all_reduce_calls'] == 6 * (nb + 2), res
    assert res['list_all_reduce_calls'] == 6 * (nb + 2), res
    assert res['captures'] == 2  # two padded shapes
    # every list: normaliser + logs (one mark each), an issue and a wait mark per
    # bucket -- in the order the eager step issues them
    assert res['plan_collectives'] == [nb + 2] * 2, res
    assert res['list_marks'] == [2 * nb + 2] * 2, res
    assert res['plan_kinds'] == ['ss' + 'i' * nb + 'w' * nb] * 2, res
    # GraphedStep(launcher='list') built directly under the group
    assert res['direct_equal'] and res['direct_marks'] == 2 * nb + 2, res
    # the hipGraphLaunch launcher cannot be cut: still refused
    assert res['default_launcher_refused'] is True


def test_auto_stepper_pipelined_list_under_process_group():
    res = _run('bf16', 'pipelined')
    assert res['raised'] is None, res['raised']
    assert res['params_equal'] and res['momentum_equal'] and res['losses_equal'], res
    nb = res['buckets']
    assert res['eager_all_reduce_calls'] == 4 * (nb + 2), res
    assert res['list_all_reduce_calls'] == 4 * (nb + 2), res
    assert res['captures'] == 1
    assert res['list_marks'] == [2 * nb + 2] * 2, res
    assert res['plan_collectives'] == [nb + 2] * 2, res
