"""The seeded 8-image dataset fixture of the dataset / loader / test-loop
tests: ``write_fixture(root)`` writes

    root/VOC2007/JPEGImages/{id}.jpg, Annotations/{id}.xml,
                 ImageSets/Main/{trainval,test}.txt
    root/middle.pkl, root/middle.json      the same annotations, middle format
    root/coco.json                         a COCO json over the same images
    root/classes.txt                       a class-name file

Everything is a pure function of ``SEED``; tools/gen_golden_datasets.py runs
the reference's dataset classes on the same tree and stores what they return in
tests/golden/datasets.npz.

Edge cases on purpose.  XML: a ``difficult`` object (000001), float
coordinates (000001), an unknown class name (000002, 000003), an image with no
valid object (000003 only unknown, 000008 none), portrait and landscape images,
one image under 32 pixels (000004), one file without ``<size>`` (000005), small
boxes for ``min_size`` (000006).  COCO: a crowd annotation, a zero-area one, a
box partly outside the image, one wholly outside, an ``ignore`` one, a
category outside CLASSES, an image without annotations, a sub-pixel box.
"""
import json
import os
import pickle

import numpy as np

SEED = 20240607
VOC_CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car',
               'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
               'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train',
               'tvmonitor')

# id, (width, height), write <size>, objects (name, difficult, xmin ymin xmax ymax)
IMAGES = [
    ('000001', (130, 100), True, [
        ('car', 0, '12', '20', '90', '77'),
        ('person', 1, '60', '10', '100', '95'),
        ('dog', 0, '5.7', '40.2', '48.9', '88.5')]),
    ('000002', (80, 120), True, [
        ('dog', 0, '10', '30', '70', '110'),
        ('unicorn', 0, '1', '1', '40', '40')]),
    ('000003', (96, 64), True, [
        ('unicorn', 0, '8', '8', '60', '50')]),
    ('000004', (40, 24), True, [
        ('cat', 0, '2', '2', '30', '20')]),
    ('000005', (100, 100), False, [
        ('cat', 0, '20', '25', '80', '90'),
        ('cat', 1, '1', '1', '30', '30')]),
    ('000006', (128, 96), True, [
        ('bicycle', 0, '30', '30', '36', '70'),
        ('bicycle', 0, '50', '20', '120', '90'),
        ('person', 0, '2', '3', '9', '11')]),
    ('000007', (64, 100), True, [
        ('person', 0, '8', '5', '55', '96'),
        ('bicycle', 1, '10', '50', '60', '99')]),
    ('000008', (110, 70), True, []),
]

COCO_CATEGORIES = [
    dict(id=1, name='person', supercategory='person'),
    dict(id=2, name='bicycle', supercategory='vehicle'),
    dict(id=3, name='car', supercategory='vehicle'),
    dict(id=18, name='dog', supercategory='animal'),
    dict(id=999, name='unicorn', supercategory='animal'),
]

# image index (into IMAGES), category id, xywh, area, extra keys
COCO_ANNS = [
    (0, 3, [12.0, 20.0, 78.0, 57.0], 4446.0, {}),
    (0, 1, [60.5, 10.25, 40.0, 85.0], 3400.0, dict(iscrowd=1)),
    (0, 18, [5.0, 40.0, 43.0, 48.0], 0.0, {}),                 # zero area
    (0, 1, [100.0, 60.0, 60.0, 70.0], 4200.0, {}),             # partly outside
    (0, 1, [140.0, 10.0, 20.0, 20.0], 400.0, {}),              # wholly outside
    (1, 18, [10.0, 30.0, 60.0, 80.0], 4800.0, {}),
    (1, 999, [1.0, 1.0, 39.0, 39.0], 1521.0, {}),              # not in CLASSES
    (1, 2, [5.0, 5.0, 0.5, 30.0], 15.0, {}),                   # w < 1
    (2, 999, [8.0, 8.0, 52.0, 42.0], 2184.0, {}),
    (3, 1, [2.0, 2.0, 28.0, 18.0], 504.0, {}),                 # tiny image
    (5, 2, [50.0, 20.0, 70.0, 70.0], 4900.0, {}),
    (5, 1, [2.0, 3.0, 7.0, 8.0], 56.0, dict(ignore=1)),
    (5, 2, [30.0, 30.0, 6.0, 40.0], 240.0, dict(iscrowd=0)),
    (6, 1, [8.0, 5.0, 47.0, 91.0], 4277.0, {}),
    (6, 2, [10.0, 50.0, 50.0, 49.0], 2450.0, dict(iscrowd=1)),
]


def _xml(img_id, size, with_size, objects):
    lines = ['<annotation>', f'  <filename>{img_id}.jpg</filename>']
    if with_size:
        lines += ['  <size>', f'    <width>{size[0]}</width>',
                  f'    <height>{size[1]}</height>', '    <depth>3</depth>',
                  '  </size>']
    for name, difficult, x1, y1, x2, y2 in objects:
        lines += ['  <object>', f'    <name>{name}</name>',
                  f'    <difficult>{difficult}</difficult>', '    <bndbox>',
                  f'      <xmin>{x1}</xmin>', f'      <ymin>{y1}</ymin>',
                  f'      <xmax>{x2}</xmax>', f'      <ymax>{y2}</ymax>',
                  '    </bndbox>', '  </object>']
    lines.append('</annotation>')
    return '\n'.join(lines) + '\n'


def middle_format():
    """The XML annotations as CustomDataset's list (classes = VOC_CLASSES,
    unknown names dropped, ``difficult`` to the ignore fields, the - 1
    offset of xml_style.py applied)."""
    out = []
    for img_id, (w, h), _, objects in IMAGES:
        b, l, bi, li = [], [], [], []
        for name, difficult, *xy in objects:
            if name not in VOC_CLASSES:
                continue
            box = [int(float(v)) - 1 for v in xy]
            (bi if difficult else b).append(box)
            (li if difficult else l).append(VOC_CLASSES.index(name))
        out.append(dict(
            filename=f'VOC2007/JPEGImages/{img_id}.jpg', width=w, height=h,
            ann=dict(
                bboxes=np.asarray(b, np.float32).reshape(-1, 4),
                labels=np.asarray(l, np.int64).reshape(-1),
                bboxes_ignore=np.asarray(bi, np.float32).reshape(-1, 4),
                labels_ignore=np.asarray(li, np.int64).reshape(-1))))
    return out


def coco_json():
    images = [dict(id=100 + 7 * k, file_name=f'VOC2007/JPEGImages/{i}.jpg',
                   width=w, height=h)
              for k, (i, (w, h), _, _) in enumerate(IMAGES)]
    anns = []
    for k, (img, cat, box, area, extra) in enumerate(COCO_ANNS):
        a = dict(id=1000 + k, image_id=images[img]['id'], category_id=cat,
                 bbox=box, area=area, iscrowd=0)
        a.update(extra)
        anns.append(a)
    return dict(images=images, annotations=anns, categories=COCO_CATEGORIES)


def write_fixture(root, seed=SEED):
    """Writes the tree under ``root`` and returns ``root``."""
    from PIL import Image
    root = str(root)
    rng = np.random.RandomState(seed)
    voc = os.path.join(root, 'VOC2007')
    for d in ('JPEGImages', 'Annotations', os.path.join('ImageSets', 'Main')):
        os.makedirs(os.path.join(voc, d), exist_ok=True)
    for img_id, (w, h), with_size, objects in IMAGES:
        # smooth blobs compress to stable JPEGs: a low-res noise field upscaled
        small = rng.randint(0, 256, size=((h + 7) // 8, (w + 7) // 8, 3))
        pix = np.kron(small, np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
        Image.fromarray(pix, 'RGB').save(
            os.path.join(voc, 'JPEGImages', f'{img_id}.jpg'), quality=90)
        with open(os.path.join(voc, 'Annotations', f'{img_id}.xml'), 'w') as f:
            f.write(_xml(img_id, (w, h), with_size, objects))
    ids = [i[0] for i in IMAGES]
    for name in ('trainval', 'test'):
        with open(os.path.join(voc, 'ImageSets', 'Main', f'{name}.txt'),
                  'w') as f:
            f.write('\n'.join(ids) + '\n')
    mid = middle_format()
    with open(os.path.join(root, 'middle.pkl'), 'wb') as f:
        pickle.dump(mid, f)
    with open(os.path.join(root, 'middle.json'), 'w') as f:
        json.dump([dict(m, ann={k: v.tolist() for k, v in m['ann'].items()})
                   for m in mid], f)
    with open(os.path.join(root, 'coco.json'), 'w') as f:
        json.dump(coco_json(), f)
    with open(os.path.join(root, 'classes.txt'), 'w') as f:
        f.write('dog\nperson\ncar\n')
    return root


def dataset_kwargs(root):
    """The constructor keywords of every run; the golden generator builds the
    reference's classes and the tests build ours from this one table."""
    voc = dict(ann_file='VOC2007/ImageSets/Main/trainval.txt',
               img_prefix='VOC2007/', data_root=root, pipeline=[])
    mid = dict(ann_file='middle.pkl', img_prefix='', data_root=root,
               pipeline=[], classes=VOC_CLASSES)
    return {
        'voc_train': ('VOCDataset', dict(voc)),
        'voc_test': ('VOCDataset', dict(voc, test_mode=True)),
        'voc_nofilter': ('VOCDataset', dict(voc, filter_empty_gt=False)),
        'voc_minsize': ('VOCDataset', dict(voc, min_size=10)),
        'xml_classes': ('XMLDataset', dict(voc, classes=('dog', 'person',
                                                         'car'))),
        'custom_train': ('CustomDataset', dict(mid)),
        'custom_test': ('CustomDataset', dict(mid, test_mode=True)),
    }


def seeded_results(num_images, num_classes, seed=SEED + 1, per_class=3):
    """``results[i][c]`` (k, 5) float32, k in 0..per_class: boxes inside a
    130 x 130 frame, scores in (0, 1)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(num_images):
        img = []
        for _ in range(num_classes):
            k = rng.randint(0, per_class + 1)
            xy = rng.uniform(0, 80, size=(k, 2))
            wh = rng.uniform(8, 50, size=(k, 2))
            sc = rng.uniform(0.01, 0.99, size=(k, 1))
            img.append(np.concatenate([xy, xy + wh, sc], 1).astype(np.float32))
        out.append(img)
    return out


def results_near_gt(dataset, seed=SEED + 2):
    """Seeded results that hit some GTs: every GT box of ``dataset`` jittered,
    plus the ``seeded_results`` noise, so that mAP is neither 0 nor 1."""
    rng = np.random.RandomState(seed)
    C = len(dataset.CLASSES)
    out = seeded_results(len(dataset), C, seed + 1, 1)
    for i in range(len(dataset)):
        ann = dataset.get_ann_info(i)
        for b, l in zip(ann['bboxes'], ann['labels']):
            jit = rng.uniform(-6, 6, size=4)
            row = np.concatenate([b + jit, [rng.uniform(0.3, 0.99)]])
            out[i][int(l)] = np.concatenate(
                [out[i][int(l)], row[None].astype(np.float32)])
    return out
