"""CPU checks of the command-line tools: every parser builds and prints its
help, the reference's argument rules fire, the unsupported options are refused
by name, publish_model drops the optimizer and adds the hash suffix."""
import hashlib
import importlib.util
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ('train', 'test', 'benchmark', 'publish_model', 'bench_loader')


def tool(name):
    spec = importlib.util.spec_from_file_location(
        f'_tool_{name}', os.path.join(REPO, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name', TOOLS)
def test_help_parses(name, capsys):
    with pytest.raises(SystemExit) as e:
        tool(name).parse_args(['--help'])
    assert e.value.code == 0
    assert 'usage:' in capsys.readouterr().out


def test_test_tool_argument_rules(capsys):
    T = tool('test')
    with pytest.raises(AssertionError, match='at least one operation'):
        T.parse_args(['c.py', 'w.pth'])
    with pytest.raises(ValueError, match='cannot be both'):
        T.parse_args(['c.py', 'w.pth', '--eval', 'mAP', '--format-only'])
    with pytest.raises(ValueError, match='pkl'):
        T.parse_args(['c.py', 'w.pth', '--out', 'r.json'])
    a = T.parse_args(['c.py', 'w.pth', '--out', 'r.pkl', '--eval', 'bbox',
                      'proposal', '--show-dir', 'd', '--show-score-thr', '0.5',
                      '--eval-options', 'classwise=True', 'iou_thr=0.75',
                      '--cfg-options', 'data.test.samples_per_gpu=2',
                      'model.bbox_head.test_cfg.score_thr=0.001',
                      'a.b=[1,2]', 'c=x,y', 'd=None', 'e=some/path.txt'])
    assert a.eval == ['bbox', 'proposal'] and a.show_score_thr == 0.5
    assert a.eval_options == dict(classwise=True, iou_thr=0.75)
    assert a.cfg_options == {
        'data.test.samples_per_gpu': 2,
        'model.bbox_head.test_cfg.score_thr': 0.001, 'a.b': [1, 2],
        'c': ['x', 'y'], 'd': None, 'e': 'some/path.txt'}
    for only in (['--out', 'r.pkl'], ['--eval', 'mAP'], ['--format-only'],
                 ['--show-dir', 'd']):
        T.parse_args(['c.py', 'w.pth'] + only)
    for opt in (['--launcher', 'pytorch'], ['--gpu-collect'],
                ['--tmpdir', 't'], ['--show'], ['--fuse-conv-bn']):
        with pytest.raises(SystemExit) as e:
            T.parse_args(['c.py', 'w.pth', '--out', 'r.pkl'] + opt)
        assert e.value.code == 2
        assert f'{opt[0]} is not supported' in capsys.readouterr().err
    assert T.parse_args(['c.py', 'w.pth', '--out', 'r.pkl', '--launcher',
                         'none']).launcher == 'none'


def test_train_and_benchmark_argument_rules(capsys):
    R = tool('train')
    a = R.parse_args(['c.py', '--work-dir', 'w', '--resume-from', 'e.pth',
                      '--no-validate', '--seed', '3', '--deterministic',
                      '--cfg-options', 'runner.max_epochs=2'])
    assert (a.work_dir, a.resume_from, a.no_validate, a.seed,
            a.deterministic) == ('w', 'e.pth', True, 3, True)
    assert a.cfg_options == {'runner.max_epochs': 2}
    d = R.parse_args(['c.py'])
    assert d.seed is None and not d.no_validate and d.work_dir is None
    with pytest.raises(SystemExit):
        R.parse_args(['c.py', '--launcher', 'slurm'])
    assert '--launcher is not supported' in capsys.readouterr().err
    B = tool('benchmark')
    b = B.parse_args(['c.py', 'w.pth'])
    assert b.log_interval == 50 and b.max_images == 2000
    assert B.NUM_WARMUP == 5
    with pytest.raises(SystemExit):
        B.parse_args(['c.py', 'w.pth', '--fuse-conv-bn'])
    assert '--fuse-conv-bn is not supported' in capsys.readouterr().err


def test_publish_model(tmp_path):
    P = tool('publish_model')
    src = str(tmp_path / 'epoch_1.pth')
    torch.save(dict(meta=dict(epoch=1, CLASSES=('a', 'b')),
                    state_dict=dict(w=torch.arange(6.0)),
                    optimizer=dict(state={}, param_groups=[dict(lr=0.1)])),
               src)
    out = P.process_checkpoint(src, str(tmp_path / 'ld_r18.pth'))
    assert os.path.dirname(out) == str(tmp_path)
    name = os.path.basename(out)
    sha = hashlib.sha256(open(out, 'rb').read()).hexdigest()
    assert name == f'ld_r18-{sha[:8]}.pth'
    assert not os.path.exists(str(tmp_path / 'ld_r18.pth'))
    ckpt = torch.load(out, map_location='cpu')
    assert 'optimizer' not in ckpt and set(ckpt) == {'meta', 'state_dict'}
    assert ckpt['meta']['CLASSES'] == ('a', 'b')
    assert torch.equal(ckpt['state_dict']['w'], torch.arange(6.0))
    assert 'optimizer' in torch.load(src, map_location='cpu')  # input kept
    P.main([src, str(tmp_path / 'again.pth')])
    assert [f for f in os.listdir(tmp_path) if f.startswith('again-')]


def test_config_dump_round_trip(tmp_path):
    from ld_amd import Config
    from ld_amd.cli import dump_config, pop_test_samples_per_gpu
    cfg = Config(dict(
        model=dict(type='GFL', backbone=dict(depth=18, out_indices=(0, 1))),
        data=dict(samples_per_gpu=2, test=dict(type='VOCDataset',
                                               samples_per_gpu=4,
                                               pipeline=[dict(type='A')])),
        evaluation=dict(interval=1, metric='mAP'), lr=0.01, name='x'))
    path = str(tmp_path / 'dumped.py')
    dump_config(cfg, path)
    back = Config.fromfile(path)
    assert dict(back._cfg_dict) == dict(cfg._cfg_dict)
    assert back.model.backbone.out_indices == (0, 1)
    assert pop_test_samples_per_gpu(back) == 4
    assert back.data.test.test_mode is True
    assert 'samples_per_gpu' not in back.data.test
    assert pop_test_samples_per_gpu(back) == 1


def test_init_detector_classes_from_checkpoint_meta(tmp_path):
    """apis/inference.py:14-49 on the CPU: CLASSES from the checkpoint meta,
    COCO's without one or without a checkpoint; the config stays on the
    model."""
    from ld_amd import Config, checkpoint, model_zoo
    from ld_amd.apis import init_detector
    from ld_amd.datasets import COCO_CLASSES
    from ld_amd.registry import build_detector
    cfg_path = tmp_path / 'gfl_r18.py'
    cfg_path.write_text('from ld_amd import model_zoo\n'
                        'model = model_zoo.gfl_detector(18)\n'
                        "data = dict(test=dict(pipeline=[]))\n")
    src = build_detector(model_zoo.gfl_detector(18))
    src.CLASSES = ('cat', 'dog')
    with_meta = str(tmp_path / 'with.pth')
    checkpoint.save_checkpoint(src, with_meta)
    bare = str(tmp_path / 'bare.pth')
    torch.save(dict(state_dict=src.state_dict(), meta=dict(epoch=1)), bare)
    m = init_detector(str(cfg_path), with_meta, device='cpu')
    assert tuple(m.CLASSES) == ('cat', 'dog') and not m.training
    assert isinstance(m.cfg, Config) and m.cfg.model.type == 'GFL'
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    with pytest.warns(UserWarning, match='COCO classes'):
        m = init_detector(Config.fromfile(str(cfg_path)), bare, device='cpu')
    assert m.CLASSES == COCO_CLASSES and len(m.CLASSES) == 80
    assert init_detector(str(cfg_path), device='cpu').CLASSES == COCO_CLASSES
    with pytest.raises(TypeError):
        init_detector(dict(model={}), device='cpu')
