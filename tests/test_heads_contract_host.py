"""Host test (no device): what checkpoints, the optimizer wire format and
GradArena's bucket order depend on, for each of the ten registered dense heads
built on the CPU with the constructor arguments of its GPU tests -- the ordered
state_dict keys, the ordered names and shapes of named_parameters, and the
order in which init_weights draws from the RNG -- against
tests/golden/heads_contract.json (tools/gen_heads_contract.py, written before
the heads were moved onto one base class).

The draw order is pinned twice after ``torch.manual_seed(0);
head.init_weights()``.  The recorded order of the normal_ draws is replayed on
this machine and every drawn parameter must equal its replay bit for bit.  The
float64 sum of every parameter must ``==`` the recorded one; for the drawn
weights that holds where normal_ itself reproduces the recording machine's
stream (it goes through SIMD math that differs by an ulp between CPU families;
``rng_probe`` tells), the constant-filled parameters compare everywhere."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))

import gen_heads_contract as G  # noqa: E402

HEADS = ['GFLHead', 'LDHead', 'ATSSGFLHead', 'LDATSSHead', 'FCOSGFLHead',
         'LDFCOSHead', 'RetinaGFLHead', 'LDRetinaHead', 'GFocalHead',
         'LDv2Head']


@pytest.fixture(scope='module')
def pinned():
    with open(G.OUT) as f:
        return json.load(f)['heads']


@pytest.fixture(scope='module')
def same_rng():
    with open(G.OUT) as f:
        return G.rng_probe() == json.load(f)['rng_probe']


def test_fixture_covers_every_registered_dense_head(pinned):
    from ld_amd import heads
    from ld_amd.registry import HEADS as REG
    registered = [k for k, v in REG.module_dict.items()
                  if v.__module__ == heads.__name__]
    assert sorted(registered) == sorted(HEADS) == sorted(pinned)
    assert sorted(G.head_configs()) == sorted(HEADS)


@pytest.mark.parametrize('name', HEADS)
def test_state_dict_parameter_and_init_order(pinned, same_rng, name):
    cfg = G.head_configs()[name]
    assert cfg['type'] == name
    want = pinned[name]
    head, draws = G.init_head(cfg)
    assert list(head.state_dict()) == want['state_dict']
    names = [n for n, _ in head.named_parameters()]
    assert [[n, list(p.shape)] for n, p in head.named_parameters()] == \
        want['parameters']
    assert draws == want['init_draws']
    assert G.replay_mismatches(head, draws) == []
    drawn = {n for n, _, _ in draws}
    assert len(want['init_sums']) == len(names) > len(drawn) > 0
    for n, p, ref in zip(names, head.parameters(), want['init_sums']):
        if same_rng or n not in drawn:
            assert G._sum64(p) == ref, n  # float64, equal, not close
