"""The reference's ``mmdet/apis``: ``single_gpu_test`` (apis/test.py:16-66),
``init_detector`` / ``inference_detector`` (apis/inference.py) over this
package's detectors, loader and device pipeline."""
import os.path as osp

import numpy as np
import torch

from .checkpoint import load_checkpoint
from .config import Config
from .datasets import COCO_CLASSES
from .pipeline import DevicePipeline
from .registry import build_detector

__all__ = ['single_gpu_test', 'init_detector', 'inference_detector',
           'feed_evaluator']


def feed_evaluator(evaluator, dataset, indices, dets):
    """One batch of device detections ``[(dets (k, 5), labels (k,)), ...]`` of
    the dataset images ``indices`` into a streaming evaluator: a
    ``CocoEvaluator`` / ``CocoProposalEvaluator`` (keyed by dataset index), a
    ``MapAccumulator`` (with the images' annotations) or a
    ``RecallAccumulator`` (detections as proposals)."""
    from .coco_eval import CocoEvaluator
    from .evaluation import MapAccumulator
    from .recall import CocoProposalEvaluator, RecallAccumulator
    boxes = [d for d, _ in dets]
    labels = [l for _, l in dets]
    if isinstance(evaluator, CocoEvaluator):
        evaluator.add(list(indices), boxes, labels)
    elif isinstance(evaluator, CocoProposalEvaluator):
        evaluator.add(list(indices), boxes)
    elif isinstance(evaluator, MapAccumulator):
        anns = [dataset.get_ann_info(i) for i in indices]
        evaluator.add(boxes, labels, [a['bboxes'] for a in anns],
                      [a['labels'] for a in anns],
                      [a.get('bboxes_ignore') for a in anns]
                      if all('bboxes_ignore' in a for a in anns) else None,
                      [a.get('labels_ignore') for a in anns]
                      if all('labels_ignore' in a for a in anns) else None)
    elif isinstance(evaluator, RecallAccumulator):
        anns = [dataset.get_ann_info(i) for i in indices]
        evaluator.add(boxes, [a['bboxes'] for a in anns])
    else:
        raise TypeError(f'single_gpu_test: evaluator {type(evaluator)}')


def single_gpu_test(model, data_loader, show_dir=None, show_score_thr=0.3,
                    evaluator=None):
    """apis/test.py:16-66: ``model(return_loss=False, rescale=True, **data)``
    per batch of ``data_loader`` (a test-mode ``DeviceDataLoader``) -> the list
    of per-image, per-class ``(k, 5)`` arrays.

    ``show_dir``: every image is drawn with ``model.show_result`` (detections
    above ``show_score_thr``) into ``show_dir/ori_filename`` with a ``.png``
    suffix.  ``evaluator``: a streaming evaluator of the dataset
    (``dataset.make_evaluator(metric)``); the device detections of every batch
    go straight into it, so its metric needs no host round trip."""
    model.eval()
    dataset = data_loader.dataset
    results = []
    # the host halves carry their dataset indices, so evaluator keys and
    # drawings belong to the images of the batch whatever the loader's order
    for host in data_loader.host_batches():
        data = data_loader.device_batch(host)
        with torch.no_grad():
            if evaluator is not None:
                result, dets = model(return_loss=False, rescale=True,
                                     return_device_dets=True, **data)
                feed_evaluator(evaluator, dataset, host['indices'], dets)
            else:
                result = model(return_loss=False, rescale=True, **data)
        assert len(result) == len(host['indices'])
        if show_dir:
            for (name, ori), res in zip(host['filenames'], result):
                model.show_result(
                    name, res, score_thr=show_score_thr,
                    out_file=osp.join(show_dir,
                                      osp.splitext(ori)[0] + '.png'))
        results.extend(result)
    return results


def init_detector(config, checkpoint=None, device='cuda:0', cfg_options=None):
    """apis/inference.py:14-49: build the detector of ``config`` (a path or a
    ``Config``), load ``checkpoint``, set ``CLASSES`` from its meta (COCO's
    otherwise), keep the config on ``model.cfg``, move to ``device``, eval."""
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError('config must be a filename or Config object, '
                        f'but got {type(config)}')
    if cfg_options is not None:
        config.merge_from_dict(cfg_options)
    mcfg = dict(config.model)
    mcfg['pretrained'] = None
    model = build_detector(mcfg, train_cfg=None,
                           test_cfg=config.get('test_cfg'))
    if checkpoint is not None:
        ckpt = load_checkpoint(model, checkpoint,
                               map_location='cpu' if device == 'cpu'
                               else None)
        if 'CLASSES' in ckpt.get('meta', {}):
            model.CLASSES = ckpt['meta']['CLASSES']
        else:
            import warnings
            warnings.warn("Class names are not saved in the checkpoint's "
                          'meta data, use COCO classes by default.')
            model.CLASSES = COCO_CLASSES
    else:
        model.CLASSES = COCO_CLASSES
    model.cfg = config
    model.to(device)
    model.eval()
    return model


def _test_pipeline(model):
    cfg = getattr(model, 'cfg', None)
    if cfg is None:
        raise ValueError('inference_detector: the model has no cfg '
                         '(build it with init_detector)')
    return cfg.data['test']['pipeline']


def inference_detector(model, imgs):
    """apis/inference.py:81-140: ``imgs`` a path or a BGR (H, W, 3) uint8
    array, or a list of them -> the per-class arrays of the image (a list of
    them for a list).  Each image is its own forward, as there with
    ``samples_per_gpu=1``."""
    from .dataloader import imread
    is_batch = isinstance(imgs, (list, tuple))
    if not is_batch:
        imgs = [imgs]
    dev = next(model.parameters()).device
    pipe = getattr(model, '_inference_pipeline', None)
    if pipe is None or pipe.device != dev:
        pipe = DevicePipeline.from_test_cfg(_test_pipeline(model), device=dev)
        model._inference_pipeline = pipe
    results = []
    for img in imgs:
        name = img if isinstance(img, str) else None
        arr = imread(img) if isinstance(img, str) else np.asarray(img)
        views, metas = pipe.aug_views(arr)
        for view in metas:
            view[0]['filename'] = view[0]['ori_filename'] = name
        with torch.no_grad():
            results.append(model(return_loss=False, rescale=True, img=views,
                                 img_metas=metas)[0])
    return results if is_batch else results[0]
