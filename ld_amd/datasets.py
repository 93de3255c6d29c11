"""Datasets: the reference's ``mmdet/datasets/{custom,xml_style,voc,coco,
dataset_wrappers,builder}.py`` restated, so that a config's ``data.train`` /
``data.val`` / ``data.test`` blocks build unchanged through
``build_dataset(cfg)``.

Constructor keywords and attribute names are the reference's (``ann_file,
pipeline, classes, data_root, img_prefix, test_mode, filter_empty_gt``;
``data_infos, flag, CLASSES, cat_ids, cat2label, img_ids``).  What differs:

* ``pipeline`` is kept as the list of dicts it is (``self.pipeline``): images
  are decoded by ``ld_amd.dataloader`` and transformed on the device by
  ``DevicePipeline``, so a dataset has no ``__getitem__`` that runs transforms;
  ``dataset[i]`` returns ``dict(img_info=..., ann_info=..., img_prefix=...)``.
* ``CocoDataset`` reads the json itself (pycocotools is not a dependency) and
  scores through ``coco_evaluate`` / ``coco_proposal_evaluate``; its index is
  unpinned against pycocotools.
* ``evaluate`` runs the device evaluators (``eval_map``, ``eval_recalls``).
* ``make_evaluator(metric)`` gives the streaming evaluator of the same metric.

Refused by name (``NotImplementedError``): ``ClassBalancedDataset``,
``proposal_file``, ``seg_prefix``, ``LoadAnnotations(with_mask / with_seg)``,
and every dataset type not defined here.
"""
import bisect
import copy
import json
import os.path as osp
import pickle
import tempfile
import warnings
import xml.etree.ElementTree as ET
from collections import OrderedDict

import numpy as np

from .registry import DATASETS, build_from_cfg

__all__ = ['CustomDataset', 'XMLDataset', 'VOCDataset', 'CocoDataset',
           'ConcatDataset', 'RepeatDataset', 'build_dataset', 'DATASETS']


def list_from_file(filename):
    """mmcv.list_from_file with its defaults: one stripped line per entry."""
    with open(filename, 'r', encoding='utf-8') as f:
        return [line.rstrip('\n\r') for line in f]


def _load(path):
    """mmcv.load for the two formats a middle-format file comes in."""
    if path.endswith('.json'):
        with open(path) as f:
            return json.load(f)
    if path.endswith(('.pkl', '.pickle')):
        with open(path, 'rb') as f:
            return pickle.load(f)
    raise TypeError(f'Unsupported annotation file format: {path}')


def _check_pipeline(pipeline):
    for step in pipeline or []:
        if step.get('type') == 'LoadAnnotations':
            for key in ('with_mask', 'with_seg'):
                if step.get(key, False):
                    raise NotImplementedError(
                        f'LoadAnnotations({key}=True): masks and semantic '
                        'maps are not loaded (bbox detection only)')


@DATASETS.register_module()
class CustomDataset:
    """custom.py:15-325: the middle-format list (``filename, width, height,
    ann``) from a ``.pkl`` or ``.json`` file."""

    CLASSES = None

    def __init__(self, ann_file, pipeline=None, classes=None, data_root=None,
                 img_prefix='', seg_prefix=None, proposal_file=None,
                 test_mode=False, filter_empty_gt=True):
        if seg_prefix is not None:
            raise NotImplementedError(
                'seg_prefix: semantic segmentation maps are not loaded')
        if proposal_file is not None:
            raise NotImplementedError(
                'proposal_file: precomputed proposals are not loaded')
        _check_pipeline(pipeline)
        self.ann_file = ann_file
        self.data_root = data_root
        self.img_prefix = img_prefix
        self.seg_prefix = None
        self.proposal_file = None
        self.proposals = None
        self.test_mode = test_mode
        self.filter_empty_gt = filter_empty_gt
        self.CLASSES = self.get_classes(classes)
        # custom.py:74-85
        if self.data_root is not None:
            if not osp.isabs(self.ann_file):
                self.ann_file = osp.join(self.data_root, self.ann_file)
            if not (self.img_prefix is None or osp.isabs(self.img_prefix)):
                self.img_prefix = osp.join(self.data_root, self.img_prefix)
        self.data_infos = self.load_annotations(self.ann_file)
        if not test_mode:
            valid_inds = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in valid_inds]
            self._set_group_flag()
        self.pipeline = list(pipeline or [])

    def __len__(self):
        return len(self.data_infos)

    def load_annotations(self, ann_file):
        infos = _load(ann_file)
        if ann_file.endswith('.json'):  # arrays come back as lists
            for info in infos:
                ann = info.get('ann')
                if ann is None:
                    continue
                for k, shape, dt in (('bboxes', (-1, 4), np.float32),
                                     ('labels', (-1, ), np.int64),
                                     ('bboxes_ignore', (-1, 4), np.float32),
                                     ('labels_ignore', (-1, ), np.int64)):
                    if k in ann:
                        ann[k] = np.asarray(ann[k], dt).reshape(shape)
        return infos

    def get_ann_info(self, idx):
        return self.data_infos[idx]['ann']

    def get_cat_ids(self, idx):
        return self.data_infos[idx]['ann']['labels'].astype(int).tolist()

    def _filter_imgs(self, min_size=32):
        if self.filter_empty_gt:
            warnings.warn(
                'CustomDataset does not support filtering empty gt images.')
        return [i for i, info in enumerate(self.data_infos)
                if min(info['width'], info['height']) >= min_size]

    def _set_group_flag(self):
        self.flag = np.zeros(len(self), dtype=np.uint8)
        for i, info in enumerate(self.data_infos):
            if info['width'] / info['height'] > 1:
                self.flag[i] = 1

    def __getitem__(self, idx):
        info = self.data_infos[idx]
        out = dict(img_info=info, img_prefix=self.img_prefix)
        if not self.test_mode:
            out['ann_info'] = self.get_ann_info(idx)
        return out

    def img_names(self, idx):
        """-> ``(filename, ori_filename)`` as LoadImageFromFile sets them:
        ``img_prefix`` joined when set, and the info's own ``filename``."""
        ori = self.data_infos[idx]['filename']
        return (osp.join(self.img_prefix, ori) if self.img_prefix is not None
                else ori), ori

    def img_path(self, idx):
        return self.img_names(idx)[0]

    @classmethod
    def get_classes(cls, classes=None):
        if classes is None:
            return cls.CLASSES
        if isinstance(classes, str):
            return list_from_file(classes)
        if isinstance(classes, (tuple, list)):
            return classes
        raise ValueError(f'Unsupported type {type(classes)} of classes.')

    def format_results(self, results, **kwargs):
        pass

    def _annotations(self):
        return [self.get_ann_info(i) for i in range(len(self))]

    def _recall(self, results, annotations, proposal_nums, iou_thr, logger):
        from .recall import eval_recalls
        iou_thrs = [iou_thr] if isinstance(iou_thr, float) else iou_thr
        gt_bboxes = [ann['bboxes'] for ann in annotations]
        recalls = eval_recalls(gt_bboxes, results, proposal_nums, iou_thr,
                               logger=logger)
        out = OrderedDict()
        for i, num in enumerate(proposal_nums):
            for j, iou in enumerate(iou_thrs):
                out[f'recall@{num}@{iou}'] = recalls[i, j]
        if recalls.shape[1] > 1:
            ar = recalls.mean(axis=1)
            for i, num in enumerate(proposal_nums):
                out[f'AR@{num}'] = ar[i]
        return out

    @staticmethod
    def _one_metric(metric):
        if not isinstance(metric, str):
            assert len(metric) == 1
            metric = metric[0]
        if metric not in ('mAP', 'recall'):
            raise KeyError(f'metric {metric} is not supported')
        return metric

    def evaluate(self, results, metric='mAP', logger=None,
                 proposal_nums=(100, 300, 1000), iou_thr=0.5,
                 scale_ranges=None):
        """custom.py:267-324 through the device ``eval_map`` /
        ``eval_recalls``."""
        from .evaluation import eval_map
        metric = self._one_metric(metric)
        annotations = self._annotations()
        if metric == 'recall':
            return self._recall(results, annotations, proposal_nums, iou_thr,
                                logger)
        eval_results = OrderedDict()
        iou_thrs = [iou_thr] if isinstance(iou_thr, float) else iou_thr
        assert isinstance(iou_thrs, list)
        mean_aps = []
        for thr in iou_thrs:
            mean_ap, _ = eval_map(results, annotations,
                                  scale_ranges=scale_ranges, iou_thr=thr,
                                  dataset=self.CLASSES, logger=logger)
            mean_aps.append(mean_ap)
            eval_results[f'AP{int(thr * 100):02d}'] = round(mean_ap, 3)
        eval_results['mAP'] = sum(mean_aps) / len(mean_aps)
        return eval_results

    def _map_dataset_name(self):
        return self.CLASSES

    def make_evaluator(self, metric='mAP', iou_thr=0.5,
                       proposal_nums=(100, 300, 1000), scale_ranges=None,
                       device=None):
        """The streaming evaluator of ``evaluate(metric=...)``: a
        ``MapAccumulator`` ('mAP') or ``RecallAccumulator`` ('recall') that
        ``single_gpu_test(evaluator=...)`` feeds batch by batch."""
        metric = self._one_metric(metric)
        if metric == 'recall':
            from .recall import RecallAccumulator
            return RecallAccumulator(proposal_nums, iou_thr, device=device)
        from .evaluation import MapAccumulator
        iou_thrs = [iou_thr] if isinstance(iou_thr, float) else list(iou_thr)
        return MapAccumulator(len(self.CLASSES), iou_thrs, scale_ranges,
                              self._map_dataset_name(), device)


@DATASETS.register_module()
class XMLDataset(CustomDataset):
    """xml_style.py:12-169.  ``min_size``: boxes smaller than it go to the
    ignored field (train mode only)."""

    def __init__(self, min_size=None, **kwargs):
        assert self.CLASSES or kwargs.get('classes', None), \
            'CLASSES in `XMLDataset` can not be None.'
        super().__init__(**kwargs)
        self.cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}
        self.min_size = min_size

    def _xml_root(self, img_id):
        path = osp.join(self.img_prefix, 'Annotations', f'{img_id}.xml')
        return ET.parse(path).getroot()

    def load_annotations(self, ann_file):
        data_infos = []
        for img_id in list_from_file(ann_file):
            filename = f'JPEGImages/{img_id}.jpg'
            size = self._xml_root(img_id).find('size')
            if size is not None:
                width = int(size.find('width').text)
                height = int(size.find('height').text)
            else:
                from PIL import Image
                with Image.open(osp.join(self.img_prefix, 'JPEGImages',
                                         f'{img_id}.jpg')) as img:
                    width, height = img.size
            data_infos.append(dict(id=img_id, filename=filename, width=width,
                                   height=height))
        return data_infos

    def _filter_imgs(self, min_size=32):
        valid_inds = []
        for i, info in enumerate(self.data_infos):
            if min(info['width'], info['height']) < min_size:
                continue
            if self.filter_empty_gt:
                for obj in self._xml_root(info['id']).findall('object'):
                    if obj.find('name').text in self.CLASSES:
                        valid_inds.append(i)
                        break
            else:
                valid_inds.append(i)
        return valid_inds

    def get_ann_info(self, idx):
        root = self._xml_root(self.data_infos[idx]['id'])
        bboxes, labels, bboxes_ignore, labels_ignore = [], [], [], []
        for obj in root.findall('object'):
            name = obj.find('name').text
            if name not in self.CLASSES:
                continue
            label = self.cat2label[name]
            difficult = int(obj.find('difficult').text)
            bnd_box = obj.find('bndbox')
            bbox = [int(float(bnd_box.find(k).text))
                    for k in ('xmin', 'ymin', 'xmax', 'ymax')]
            ignore = False
            if self.min_size:
                assert not self.test_mode
                w = bbox[2] - bbox[0]
                h = bbox[3] - bbox[1]
                if w < self.min_size or h < self.min_size:
                    ignore = True
            if difficult or ignore:
                bboxes_ignore.append(bbox)
                labels_ignore.append(label)
            else:
                bboxes.append(bbox)
                labels.append(label)

        def arrays(b, l):
            if not b:  # the - 1 offset is applied to non-empty arrays only
                return np.zeros((0, 4)), np.zeros((0, ))
            return np.array(b, ndmin=2) - 1, np.array(l)

        bboxes, labels = arrays(bboxes, labels)
        bboxes_ignore, labels_ignore = arrays(bboxes_ignore, labels_ignore)
        return dict(bboxes=bboxes.astype(np.float32),
                    labels=labels.astype(np.int64),
                    bboxes_ignore=bboxes_ignore.astype(np.float32),
                    labels_ignore=labels_ignore.astype(np.int64))

    def get_cat_ids(self, idx):
        root = self._xml_root(self.data_infos[idx]['id'])
        return [self.cat2label[obj.find('name').text]
                for obj in root.findall('object')
                if obj.find('name').text in self.CLASSES]


@DATASETS.register_module()
class VOCDataset(XMLDataset):
    """voc.py:6-101."""

    CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car',
               'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
               'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train',
               'tvmonitor')

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if 'VOC2007' in self.img_prefix:
            self.year = 2007
        elif 'VOC2012' in self.img_prefix:
            self.year = 2012
        else:
            raise ValueError('Cannot infer dataset year from img_prefix')

    def _map_dataset_name(self):
        return 'voc07' if self.year == 2007 else self.CLASSES

    def evaluate(self, results, metric='mAP', logger=None,
                 proposal_nums=(100, 300, 1000), iou_thr=0.5,
                 scale_ranges=None, ap_range=False):
        """voc.py:23-101: ``mAP`` is ``eval_map`` at ``iou_thr`` with the
        11-point AP for VOC2007 and the area AP otherwise; that is all the
        reference returns, and one evaluation gives it.  The reference also
        PRINTS the mAP at ``iou_thr + 0.05 k``, k < 10, and their mean;
        ``ap_range=True`` prints the same lines from ONE accumulation over the
        ten thresholds (the reference's own accumulated floats) and adds them
        to the result as ``AP50`` ... ``AP95`` and ``AP``."""
        from .evaluation import MapAccumulator, eval_map
        metric = self._one_metric(metric)
        annotations = self._annotations()
        if metric == 'recall':
            return dict(self._recall(results, annotations, proposal_nums,
                                     iou_thr, logger))
        assert isinstance(iou_thr, float)
        name = self._map_dataset_name()
        if not ap_range:
            mean_ap, _ = eval_map(results, annotations, scale_ranges=None,
                                  iou_thr=iou_thr, dataset=name, logger=logger)
            return {'mAP': mean_ap}
        thrs = [iou_thr]
        for _ in range(9):
            thrs.append(thrs[-1] + 0.05)  # voc.py:78, the same sums
        acc = MapAccumulator(len(results[0]), thrs, None, name)
        acc.add_results(results, annotations)
        maps = [m for m, _ in acc.compute(logger)]
        eval_results = {'mAP': maps[0]}
        for k, m in enumerate(maps):
            eval_results[f'AP{int(50 + 5 * k)}'] = m
        eval_results['AP'] = sum(maps) / 10
        if logger != 'silent':
            print([f'{k}: {v:.6f}' for k, v in eval_results.items()
                   if k != 'mAP'])
        return eval_results


COCO_CLASSES = (
    'person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train',
    'truck', 'boat', 'traffic light', 'fire hydrant', 'stop sign',
    'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow',
    'elephant', 'bear', 'zebra', 'giraffe', 'backpack', 'umbrella', 'handbag',
    'tie', 'suitcase', 'frisbee', 'skis', 'snowboard', 'sports ball', 'kite',
    'baseball bat', 'baseball glove', 'skateboard', 'surfboard',
    'tennis racket', 'bottle', 'wine glass', 'cup', 'fork', 'knife', 'spoon',
    'bowl', 'banana', 'apple', 'sandwich', 'orange', 'broccoli', 'carrot',
    'hot dog', 'pizza', 'donut', 'cake', 'chair', 'couch', 'potted plant',
    'bed', 'dining table', 'toilet', 'tv', 'laptop', 'mouse', 'remote',
    'keyboard', 'cell phone', 'microwave', 'oven', 'toaster', 'sink',
    'refrigerator', 'book', 'clock', 'vase', 'scissors', 'teddy bear',
    'hair drier', 'toothbrush')


@DATASETS.register_module()
class CocoDataset(CustomDataset):
    """coco.py:29-545 on an index of its own: ``cat_ids`` in ``CLASSES``
    order (names the json does not have are left out), ``img_ids`` in the
    json's ``images`` order, an image's annotations in the json's order."""

    CLASSES = COCO_CLASSES

    def load_annotations(self, ann_file):
        with open(ann_file) as f:
            self.coco_dict = json.load(f)
        by_name = {c['name']: c['id']
                   for c in self.coco_dict.get('categories', [])}
        self.cat_ids = [by_name[n] for n in self.CLASSES if n in by_name]
        self.cat_names = [n for n in self.CLASSES if n in by_name]
        self.cat2label = {cat_id: i for i, cat_id in enumerate(self.cat_ids)}
        self.img_ids = [im['id'] for im in self.coco_dict.get('images', [])]
        self.img_to_anns = {i: [] for i in self.img_ids}
        self.cat_img_map = {}
        for ann in self.coco_dict.get('annotations', []):
            self.img_to_anns.setdefault(ann['image_id'], []).append(ann)
            self.cat_img_map.setdefault(ann['category_id'], []).append(
                ann['image_id'])
        data_infos = []
        for im in self.coco_dict.get('images', []):
            info = dict(im)
            info['filename'] = info['file_name']
            data_infos.append(info)
        self._gt = None
        return data_infos

    def get_ann_info(self, idx):
        info = self.data_infos[idx]
        return self._parse_ann_info(info, self.img_to_anns[info['id']])

    def get_cat_ids(self, idx):
        return [ann['category_id']
                for ann in self.img_to_anns[self.data_infos[idx]['id']]]

    def _filter_imgs(self, min_size=32):
        """coco.py:98-120; rewrites ``img_ids`` to stay aligned with
        ``data_infos``."""
        ids_with_ann = set(a['image_id']
                           for a in self.coco_dict.get('annotations', []))
        ids_in_cat = set()
        for class_id in self.cat_ids:
            ids_in_cat |= set(self.cat_img_map.get(class_id, []))
        ids_in_cat &= ids_with_ann
        valid_inds, valid_img_ids = [], []
        for i, info in enumerate(self.data_infos):
            img_id = self.img_ids[i]
            if self.filter_empty_gt and img_id not in ids_in_cat:
                continue
            if min(info['width'], info['height']) >= min_size:
                valid_inds.append(i)
                valid_img_ids.append(img_id)
        self.img_ids = valid_img_ids
        return valid_inds

    def _parse_ann_info(self, img_info, ann_info):
        """coco.py:122-179 without the mask fields."""
        gt_bboxes, gt_labels, gt_bboxes_ignore = [], [], []
        for ann in ann_info:
            if ann.get('ignore', False):                      # coco.py:139
                continue
            x1, y1, w, h = ann['bbox']
            inter_w = max(0, min(x1 + w, img_info['width']) - max(x1, 0))
            inter_h = max(0, min(y1 + h, img_info['height']) - max(y1, 0))
            if inter_w * inter_h == 0:                        # coco.py:144
                continue
            if ann['area'] <= 0 or w < 1 or h < 1:            # coco.py:146
                continue
            if ann['category_id'] not in self.cat_ids:        # coco.py:148
                continue
            bbox = [x1, y1, x1 + w, y1 + h]
            if ann.get('iscrowd', False):                     # coco.py:151
                gt_bboxes_ignore.append(bbox)
            else:
                gt_bboxes.append(bbox)
                gt_labels.append(self.cat2label[ann['category_id']])
        if gt_bboxes:
            gt_bboxes = np.array(gt_bboxes, dtype=np.float32)
            gt_labels = np.array(gt_labels, dtype=np.int64)
        else:
            gt_bboxes = np.zeros((0, 4), dtype=np.float32)
            gt_labels = np.array([], dtype=np.int64)
        if gt_bboxes_ignore:
            gt_bboxes_ignore = np.array(gt_bboxes_ignore, dtype=np.float32)
        else:
            gt_bboxes_ignore = np.zeros((0, 4), dtype=np.float32)
        return dict(bboxes=gt_bboxes, labels=gt_labels,
                    bboxes_ignore=gt_bboxes_ignore,
                    seg_map=img_info['filename'].replace('jpg', 'png'))

    # -- results -> json ------------------------------------------------------
    def xyxy2xywh(self, bbox):
        _bbox = bbox.tolist()
        return [_bbox[0], _bbox[1], _bbox[2] - _bbox[0], _bbox[3] - _bbox[1]]

    def _proposal2json(self, results):
        out = []
        for idx in range(len(self)):
            for b in results[idx]:
                out.append(dict(image_id=self.img_ids[idx],
                                bbox=self.xyxy2xywh(b), score=float(b[4]),
                                category_id=1))
        return out

    def _det2json(self, results):
        out = []
        for idx in range(len(self)):
            for label, bboxes in enumerate(results[idx]):
                for b in bboxes:
                    out.append(dict(image_id=self.img_ids[idx],
                                    bbox=self.xyxy2xywh(b), score=float(b[4]),
                                    category_id=self.cat_ids[label]))
        return out

    def results2json(self, results, outfile_prefix):
        """coco.py:271-309 for bbox lists and proposal arrays."""
        result_files = dict()
        if isinstance(results[0], list):
            result_files['bbox'] = f'{outfile_prefix}.bbox.json'
            result_files['proposal'] = f'{outfile_prefix}.bbox.json'
            with open(result_files['bbox'], 'w') as f:
                json.dump(self._det2json(results), f)
        elif isinstance(results[0], tuple):
            raise NotImplementedError(
                'results2json: (bbox, segm) results -- masks are not handled')
        elif isinstance(results[0], np.ndarray):
            result_files['proposal'] = f'{outfile_prefix}.proposal.json'
            with open(result_files['proposal'], 'w') as f:
                json.dump(self._proposal2json(results), f)
        else:
            raise TypeError('invalid type of results')
        return result_files

    def format_results(self, results, jsonfile_prefix=None, **kwargs):
        assert isinstance(results, list), 'results must be a list'
        assert len(results) == len(self), (
            'The length of results is not equal to the dataset len: {} != {}'.
            format(len(results), len(self)))
        if jsonfile_prefix is None:
            tmp_dir = tempfile.TemporaryDirectory()
            jsonfile_prefix = osp.join(tmp_dir.name, 'results')
        else:
            tmp_dir = None
        return self.results2json(results, jsonfile_prefix), tmp_dir

    def json2results(self, json_file):
        """The inverse of ``_det2json``: a bbox json -> ``results[i][c]`` (k, 5)
        float32 arrays in this dataset's image and class order."""
        with open(json_file) as f:
            dets = json.load(f)
        rank = {i: k for k, i in enumerate(self.img_ids)}
        rows = [[[] for _ in self.cat_ids] for _ in self.img_ids]
        for d in dets:
            x, y, w, h = d['bbox']
            rows[rank[d['image_id']]][self.cat2label[d['category_id']]].append(
                [x, y, x + w, y + h, d['score']])
        return [[np.asarray(r, np.float32).reshape(-1, 5) for r in img]
                for img in rows]

    # -- evaluation -----------------------------------------------------------
    def ground_truth(self):
        """The ``CocoGroundTruth`` of this dataset's images (``img_ids``
        order) and categories (``cat_ids`` order)."""
        if self._gt is None or self._gt.img_ids != list(self.img_ids):
            from .coco_eval import CocoGroundTruth
            cats = {c['id']: c for c in self.coco_dict.get('categories', [])}
            anns = self.coco_dict.get('annotations', [])
            sup = [cats[c].get('supercategory') for c in self.cat_ids]
            self._gt = CocoGroundTruth(
                self.img_ids, self.cat_ids, self.cat_names,
                [a['image_id'] for a in anns],
                [a['category_id'] for a in anns],
                np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4),
                [a['area'] for a in anns],
                [a.get('iscrowd', 0) for a in anns], [a['id'] for a in anns],
                sup if all(s is not None for s in sup) else None)
        return self._gt

    def evaluate(self, results, metric='bbox', logger=None,
                 jsonfile_prefix=None, classwise=False,
                 proposal_nums=(100, 300, 1000), iou_thrs=None,
                 metric_items=None):
        """coco.py:363-545 through ``coco_evaluate`` (bbox) and
        ``coco_proposal_evaluate`` (proposal, proposal_fast).  With
        ``jsonfile_prefix`` the bbox json is written as the reference does."""
        from .coco_eval import coco_evaluate
        from .recall import coco_proposal_evaluate
        metrics = metric if isinstance(metric, list) else [metric]
        for m in metrics:
            if m not in ('bbox', 'segm', 'proposal', 'proposal_fast'):
                raise KeyError(f'metric {m} is not supported')
            if m == 'segm':
                raise NotImplementedError(
                    "metric 'segm': masks are not handled (bbox detection "
                    'only)')
        assert isinstance(results, list), 'results must be a list'
        assert len(results) == len(self), (
            'The length of results is not equal to the dataset len: {} != {}'.
            format(len(results), len(self)))
        if jsonfile_prefix is not None:
            self.results2json(results, jsonfile_prefix)
        gt = self.ground_truth()
        eval_results = OrderedDict()
        for m in metrics:
            if m == 'bbox':
                eval_results.update(coco_evaluate(
                    results, gt, 'bbox', logger, classwise, proposal_nums,
                    iou_thrs, metric_items))
            else:
                eval_results.update(coco_proposal_evaluate(
                    results, gt, m, proposal_nums, iou_thrs, metric_items,
                    logger))
        return eval_results

    def make_evaluator(self, metric='bbox', proposal_nums=(100, 300, 1000),
                       iou_thrs=None, device=None):
        """``CocoEvaluator`` ('bbox') or ``CocoProposalEvaluator``."""
        if not isinstance(metric, str):
            assert len(metric) == 1
            metric = metric[0]
        if metric == 'bbox':
            from .coco_eval import CocoEvaluator
            return CocoEvaluator(self.ground_truth(), iou_thrs, proposal_nums,
                                 device)
        if metric in ('proposal', 'proposal_fast'):
            from .recall import CocoProposalEvaluator
            return CocoProposalEvaluator(self.ground_truth(), metric,
                                         proposal_nums, iou_thrs, device)
        raise KeyError(f'metric {metric} is not supported')


# ---------------------------------------------------------------------------
# wrappers (dataset_wrappers.py)
# ---------------------------------------------------------------------------
@DATASETS.register_module()
class ConcatDataset:
    """dataset_wrappers.py:13-124: concatenated ``flag``, the first dataset's
    ``CLASSES``, per-dataset evaluation with ``separate_eval=True``."""

    def __init__(self, datasets, separate_eval=True):
        self.datasets = list(datasets)
        assert len(self.datasets) > 0, \
            'datasets should not be an empty iterable'
        self.cumulative_sizes = list(np.cumsum(
            [len(d) for d in self.datasets]).tolist())
        self.CLASSES = self.datasets[0].CLASSES
        self.separate_eval = separate_eval
        if not separate_eval:
            if any(isinstance(ds, CocoDataset) for ds in self.datasets):
                raise NotImplementedError(
                    'Evaluating concatenated CocoDataset as a whole is not'
                    ' supported! Please set "separate_eval=True"')
            if len(set(type(ds) for ds in self.datasets)) != 1:
                raise NotImplementedError(
                    'All the datasets should have same types')
        if hasattr(self.datasets[0], 'flag'):
            self.flag = np.concatenate([d.flag for d in self.datasets])

    def __len__(self):
        return self.cumulative_sizes[-1]

    def locate(self, idx):
        """-> (dataset index, sample index) of ``idx``."""
        if idx < 0:
            if -idx > len(self):
                raise ValueError(
                    'absolute value of index should not exceed dataset length')
            idx = len(self) + idx
        d = bisect.bisect_right(self.cumulative_sizes, idx)
        return d, idx if d == 0 else idx - self.cumulative_sizes[d - 1]

    def __getitem__(self, idx):
        d, s = self.locate(idx)
        return self.datasets[d][s]

    def get_cat_ids(self, idx):
        d, s = self.locate(idx)
        return self.datasets[d].get_cat_ids(s)

    def get_ann_info(self, idx):
        d, s = self.locate(idx)
        return self.datasets[d].get_ann_info(s)

    def img_names(self, idx):
        d, s = self.locate(idx)
        return self.datasets[d].img_names(s)

    def img_path(self, idx):
        return self.img_names(idx)[0]

    @property
    def data_infos(self):
        return sum([d.data_infos for d in self.datasets], [])

    @property
    def pipeline(self):
        return self.datasets[0].pipeline

    @property
    def test_mode(self):
        return self.datasets[0].test_mode

    def evaluate(self, results, logger=None, **kwargs):
        assert len(results) == self.cumulative_sizes[-1], \
            ('Dataset and results have different sizes: '
             f'{self.cumulative_sizes[-1]} v.s. {len(results)}')
        if self.separate_eval:
            total, start = dict(), 0
            for k, (end, ds) in enumerate(zip(self.cumulative_sizes,
                                              self.datasets)):
                per = ds.evaluate(results[start:end], logger=logger, **kwargs)
                start = end
                for key, v in per.items():
                    total[f'{k}_{key}'] = v
            return total
        first = self.datasets[0]
        original = first.data_infos
        first.data_infos = sum([d.data_infos for d in self.datasets], [])
        try:
            return first.evaluate(results, logger=logger, **kwargs)
        finally:
            first.data_infos = original


@DATASETS.register_module()
class RepeatDataset:
    """dataset_wrappers.py:127-167."""

    def __init__(self, dataset, times):
        self.dataset = dataset
        self.times = times
        self.CLASSES = dataset.CLASSES
        if hasattr(self.dataset, 'flag'):
            self.flag = np.tile(self.dataset.flag, times)
        self._ori_len = len(self.dataset)

    def __getitem__(self, idx):
        return self.dataset[idx % self._ori_len]

    def get_cat_ids(self, idx):
        return self.dataset.get_cat_ids(idx % self._ori_len)

    def get_ann_info(self, idx):
        return self.dataset.get_ann_info(idx % self._ori_len)

    def img_names(self, idx):
        return self.dataset.img_names(idx % self._ori_len)

    def img_path(self, idx):
        return self.img_names(idx)[0]

    @property
    def pipeline(self):
        return self.dataset.pipeline

    @property
    def test_mode(self):
        return self.dataset.test_mode

    def __len__(self):
        return self.times * self._ori_len


# ---------------------------------------------------------------------------
# builder.py:26-73
# ---------------------------------------------------------------------------
def _concat_dataset(cfg, default_args=None):
    ann_files = cfg['ann_file']
    img_prefixes = cfg.get('img_prefix', None)
    datasets = []
    for i in range(len(ann_files)):
        data_cfg = copy.deepcopy(dict(cfg))
        data_cfg.pop('separate_eval', None)
        data_cfg['ann_file'] = ann_files[i]
        if isinstance(img_prefixes, (list, tuple)):
            data_cfg['img_prefix'] = img_prefixes[i]
        for key in ('seg_prefix', 'proposal_file'):
            if isinstance(cfg.get(key, None), (list, tuple)):
                raise NotImplementedError(f'{key}: not loaded')
        datasets.append(build_dataset(data_cfg, default_args))
    return ConcatDataset(datasets, cfg.get('separate_eval', True))


def build_dataset(cfg, default_args=None):
    if isinstance(cfg, (list, tuple)):
        return ConcatDataset([build_dataset(c, default_args) for c in cfg])
    t = cfg['type']
    if t == 'ConcatDataset':
        return ConcatDataset(
            [build_dataset(c, default_args) for c in cfg['datasets']],
            cfg.get('separate_eval', True))
    if t == 'RepeatDataset':
        return RepeatDataset(build_dataset(cfg['dataset'], default_args),
                             cfg['times'])
    if t == 'ClassBalancedDataset':
        raise NotImplementedError(
            'ClassBalancedDataset: repeat-factor sampling is not implemented')
    if isinstance(t, str) and DATASETS.get(t) is None:
        raise NotImplementedError(
            f'dataset type {t}: only {sorted(DATASETS.module_dict)} are '
            'implemented')
    if isinstance(cfg.get('ann_file'), (list, tuple)):
        return _concat_dataset(cfg, default_args)
    return build_from_cfg(dict(cfg), DATASETS, default_args)
