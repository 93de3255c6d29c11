"""CPU checks of test-time augmentation: the view expansion of
DevicePipeline.from_test_cfg against the order the reference's
MultiScaleFlipAug emits, the bbox_mapping_back restatement against the
reference's merged boxes (tests/golden/augtest.npz), and the new C ABI
(declared, exported, host-side validation of the view descriptors)."""
import ctypes
import os
import re

import numpy as np
import pytest

from ld_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NORM = dict(type='Normalize', mean=[123.675, 116.28, 103.53],
            std=[58.395, 57.12, 57.375], to_rgb=True)


def _test_pipeline(img_scale, flip=True, flip_direction='horizontal'):
    return [
        dict(type='LoadImageFromFile'),
        dict(type='MultiScaleFlipAug', img_scale=img_scale, flip=flip,
             flip_direction=flip_direction,
             transforms=[dict(type='Resize', keep_ratio=True),
                         dict(type='RandomFlip'), NORM,
                         dict(type='Pad', size_divisor=32),
                         dict(type='ImageToTensor', keys=['img']),
                         dict(type='Collect', keys=['img'])])]


def test_view_order_and_metas_vs_reference(golden):
    from ld_amd.pipeline import DevicePipeline, rescale_size
    g = golden['augtest']
    scales = [tuple(int(v) for v in s) for s in g['order_img_scale']]
    pipe = DevicePipeline.from_test_cfg(_test_pipeline(scales), device='cpu')
    plans = pipe.view_plans((480, 640))
    assert [p['scale'] for p in plans] == \
        [tuple(int(v) for v in s) for s in g['order_scale']]
    assert [p['flip'] for p in plans] == g['order_flip'].tolist()
    assert [str(p['flip_direction']) for p in plans] == \
        g['order_flip_direction'].tolist()
    for p in plans:
        new_w, new_h = rescale_size((640, 480), p['scale'])
        assert p['img_shape'] == (new_h, new_w, 3)
        assert p['ori_shape'] == (480, 640, 3)
        np.testing.assert_array_equal(
            p['scale_factor'],
            np.array([new_w / 640, new_h / 480] * 2, np.float32))
    # without flip: one view per scale
    pipe = DevicePipeline.from_test_cfg(_test_pipeline(scales, flip=False),
                                        device='cpu')
    assert [(p['scale'], p['flip']) for p in pipe.view_plans((480, 640))] == \
        [(scales[0], False), (scales[1], False)]


@pytest.mark.parametrize('direction', ['vertical', 'diagonal',
                                       ['horizontal', 'vertical']])
def test_pipeline_refuses_other_flip_directions(direction):
    from ld_amd.pipeline import DevicePipeline
    with pytest.raises(NotImplementedError, match='horizontally'):
        DevicePipeline.from_test_cfg(
            _test_pipeline((1333, 800), flip_direction=direction),
            device='cpu')


def _map_back(b, shape, sf, flip, direction):
    """bbox_flip then a true fp32 division by scale_factor
    (transforms.py:5-55), restated in numpy."""
    b = b.astype(np.float32)
    out = b.copy()
    h, w = np.float32(shape[0]), np.float32(shape[1])
    if flip and direction in ('horizontal', 'diagonal'):
        out[:, 0], out[:, 2] = w - b[:, 2], w - b[:, 0]
    if flip and direction in ('vertical', 'diagonal'):
        out[:, 1], out[:, 3] = h - b[:, 3], h - b[:, 1]
    return out / np.asarray(sf, np.float32)


@pytest.mark.parametrize('name', ['gfl_small', 'gfl_flips'])
def test_map_back_restatement_vs_reference(golden, name):
    g = golden['augtest']
    case = [c for c in synthetic.AUG_CASES if c[0] == name][0]
    metas = synthetic.aug_view_metas(case)
    mapped = [_map_back(g[f'{name}_pre_bboxes_{v}'], m[0]['img_shape'],
                        m[0]['scale_factor'], m[0]['flip'],
                        m[0]['flip_direction'])
              for v, m in enumerate(metas)]
    # the merged index is view-major (merge_aug_bboxes' torch.cat)
    np.testing.assert_array_equal(np.concatenate(mapped),
                                  g[f'{name}_merged_bboxes'])


def _declared():
    src = open(os.path.join(REPO, 'include', 'ld_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\b(ld_[a-z0-9_]+)\s*\(', src))


def test_aug_symbols_declared_and_exported():
    from ld_amd import lib as L
    names = {'ld_aug_merge_nms', 'ld_aug_merge_nms_workspace_bytes'}
    assert names <= _declared()
    assert names <= set(L.SIGNATURES)
    if not L.lib_available():
        import __graft_entry__
        __graft_entry__.build()
    so = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(so, n), n
    # ld_aug_view_t: 3 pointers, 4 int32, 6 floats
    assert ctypes.sizeof(L.AugViewT) == 64
    assert L.AugViewT.img_h.offset == 40


def test_aug_descriptor_validation_without_gpu():
    """The workspace query validates the view descriptors on the host."""
    from ld_amd import lib as L
    lib = L.get_lib()
    arr = (L.AugViewT * 3)()
    for v in range(3):
        arr[v].boxes, arr[v].scores = 0x1000, 0x2000
        arr[v].K, arr[v].score_stride = 100 + v, 81
        arr[v].scale_factor[:] = [1.0] * 4
    ws = lib.ld_aug_merge_nms_workspace_bytes(arr, 3, 80)
    # the candidate keys of every (row, class) pair + fixed parts
    assert ws >= 303 * 80 * 8
    assert lib.ld_aug_merge_nms_workspace_bytes(arr, 3, 82) == 0  # stride < C
    assert lib.ld_aug_merge_nms_workspace_bytes(arr, 0, 80) == 0
    assert lib.ld_aug_merge_nms_workspace_bytes(
        arr, L.LD_MAX_AUG_VIEWS + 1, 80) == 0
    arr[1].factors = 0x3000  # factors on some views only
    assert lib.ld_aug_merge_nms_workspace_bytes(arr, 3, 80) == 0
    arr[1].factors = None
    arr[2].flip = 4
    assert lib.ld_aug_merge_nms_workspace_bytes(arr, 3, 80) == 0
    arr[2].flip = L.LD_FLIP['diagonal']
    assert lib.ld_aug_merge_nms_workspace_bytes(arr, 3, 80) == ws
