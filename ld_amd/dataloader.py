"""The loader between a dataset and the device pipeline: the reference's
``build_dataloader`` (mmdet/datasets/builder.py:76-140) with the work split the
way this package runs it.

    host threads    order (GroupSampler / DistributedGroupSampler), JPEG decode
                    (PIL), the per-image random draws (``DevicePipeline.plan``)
    device          Resize, flip, Normalize, Pad, collate: one
                    ``ld_preprocess_batch`` launch per batch (``DevicePipeline``)

**Decode** happens on the host with PIL, on a pool of ``min(workers_per_gpu *
2, 16)`` threads -- never sized by the machine's CPU count, and threads only:
a process that has opened the GPU must not be forked.  (The device JPEG half
is out until the cause of its fault is found)  Pixels
become 3-channel BGR uint8 HWC, ``LoadImageFromFile(color_type='color')``; EXIF
orientation is applied as ``cv2.IMREAD_COLOR`` does, through
``ImageOps.exif_transpose``.  Pixel parity with cv2's decoder is NOT pinned
(libjpeg builds differ in their IDCT and chroma upsampling).

**Determinism.**  The order of epoch ``e`` comes from the sampler seeded with
``(seed, e)``; the random scale and flip draws of batch ``b`` come from
``RandomState(batch_seed(seed, e, b))``.  A batch is a pure function of
``(seed, epoch, index)``, whatever the thread timing.  With a RandomCrop in
the pipeline an image can be rejected (no gt box left); its replacement is
drawn from the same generator, so the rule still holds, and the indices a
batch really holds are ``host['indices']``.  ``seed=None`` leaves
both to numpy's global generator, as the reference does.

The loader has started at most two batches beyond the one it last handed out
(``LOOK_AHEAD``), and is itself ``make_epoch_batches`` for ``EpochRunner``
(``loader(epoch)``).  The runner's own one-batch look-ahead comes on top: while
it steps batch ``k`` it already holds ``k + 1``, so decode may have reached
``k + 3``.
"""
import hashlib
import math
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .pipeline import DevicePipeline, DistributedGroupSampler, GroupSampler

__all__ = ['imread', 'batch_seed', 'build_dataloader', 'DeviceDataLoader',
           'VirtualRankLoader']

MAX_THREADS = 16
LOOK_AHEAD = 2
MAX_REPLACEMENTS = 1000  # of one rejected image, before giving up


def imread(path):
    """A file -> (H, W, 3) uint8 BGR, EXIF orientation applied: what
    ``mmcv.imread(path, 'color')`` returns, up to the JPEG decoder."""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)
        rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def batch_seed(seed, epoch, index):
    """The 32-bit seed of batch ``index`` of epoch ``epoch``: the first four
    bytes of sha256 of the three numbers (Python's ``hash`` is salted per
    process)."""
    h = hashlib.sha256(f'{int(seed)},{int(epoch)},{int(index)}'.encode())
    return int.from_bytes(h.digest()[:4], 'little')


def threads_for_workers(workers_per_gpu):
    """min(workers_per_gpu * 2, 16), at least 1."""
    return max(1, min(int(workers_per_gpu) * 2, MAX_THREADS))


def _is_multi_view(pipe):
    return len(getattr(pipe, 'aug_scales', [None])) * \
        len(getattr(pipe, 'aug_flips', [None])) > 1


class DeviceDataLoader:
    """Iterating gives the device batches of the current epoch; ``loader(e)``
    sets the epoch first.

    Train mode (``dataset.test_mode`` false): dicts of ``img, img_metas,
    gt_bboxes, gt_labels, gt_bboxes_ignore`` from
    ``DevicePipeline.from_cfg(dataset.pipeline)``.  Test mode: dicts of ``img``
    (list of view tensors) and ``img_metas`` (list of per-view meta lists) as
    ``forward_test`` takes them, from ``DevicePipeline.from_test_cfg``: a
    single-view pipeline gives ``samples_per_gpu`` images per launch, a
    multi-view ``MultiScaleFlipAug`` one image per step (``aug_views``).
    The metas carry ``filename`` and ``ori_filename``.

    The host half is usable without a device: ``epoch_order``,
    ``batch_indices`` and ``host_batch``."""

    def __init__(self, dataset, samples_per_gpu=1, workers_per_gpu=1,
                 dist=False, shuffle=True, seed=None, device=None,
                 num_replicas=None, rank=None, num_threads=None):
        self.dataset = dataset
        self.samples_per_gpu = int(samples_per_gpu)
        # ``num_threads=`` names the pool size itself (1 .. 16) instead of
        # deriving it from workers_per_gpu
        if num_threads is None:
            self.num_threads = threads_for_workers(workers_per_gpu)
        else:
            if int(num_threads) < 1:
                raise ValueError('DeviceDataLoader: num_threads must be >= 1')
            self.num_threads = min(int(num_threads), MAX_THREADS)
        self.dist = bool(dist)
        self.shuffle = bool(shuffle)
        self.seed = seed
        self.epoch = 0
        self.test_mode = bool(getattr(dataset, 'test_mode', False))
        if self.test_mode:
            self.pipeline = DevicePipeline.from_test_cfg(dataset.pipeline,
                                                         device=device)
        else:
            self.pipeline = DevicePipeline.from_cfg(dataset.pipeline,
                                                    device=device)
        self.multi_view = self.test_mode and _is_multi_view(self.pipeline)
        # a multi-view test step is one image: aug_test takes no batch
        self.batch_size = 1 if self.multi_view else self.samples_per_gpu
        if self.dist and (num_replicas is None or rank is None):
            import torch.distributed as td
            on = td.is_available() and td.is_initialized()
            if num_replicas is None:
                num_replicas = td.get_world_size() if on else 1
            if rank is None:
                rank = td.get_rank() if on else 0
        self.num_replicas = num_replicas or 1
        self.rank = rank or 0
        self._sampler = None
        if self.shuffle and self.dist:
            self._sampler = DistributedGroupSampler(
                dataset, self.samples_per_gpu, self.num_replicas, self.rank,
                seed=seed)
        elif self.shuffle:
            self._sampler = GroupSampler(dataset, self.samples_per_gpu)
        self._pool = None

    # -- host half ------------------------------------------------------------
    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def epoch_order(self, epoch=None):
        """The dataset indices of one epoch, in the order they are used."""
        epoch = self.epoch if epoch is None else int(epoch)
        n = len(self.dataset)
        if not self.shuffle:
            if not self.dist:
                return list(range(n))
            # DistributedSampler(shuffle=False): padded, then rank::world
            per = int(math.ceil(n / self.num_replicas))
            idx = list(range(n))
            idx += idx[:per * self.num_replicas - n]
            return idx[self.rank::self.num_replicas]
        if self.dist:
            self._sampler.set_epoch(epoch)
            return list(self._sampler)
        if self.seed is None:  # numpy's global generator, as the reference
            return list(self._sampler)
        state = np.random.get_state()
        try:
            np.random.seed(batch_seed(self.seed, epoch, -1))
            return list(self._sampler)
        finally:
            np.random.set_state(state)

    def __len__(self):
        if self._sampler is not None:
            n = len(self._sampler)
        elif self.dist:
            n = int(math.ceil(len(self.dataset) / self.num_replicas))
        else:
            n = len(self.dataset)
        return int(math.ceil(n / self.batch_size))

    def batch_indices(self, order, index):
        lo = index * self.batch_size
        return order[lo:lo + self.batch_size]

    def _decode(self, idx):
        return imread(self.dataset.img_path(idx))

    def _submit(self, order, epoch, index):
        """Start decoding batch ``index``; the rest of the host half runs in
        ``_finish`` once the pixels are there."""
        idxs = self.batch_indices(order, index)
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.num_threads,
                                            thread_name_prefix='ld-decode')
        return idxs, epoch, index, [self._pool.submit(self._decode, i)
                                    for i in idxs]

    def _finish(self, job):
        idxs, epoch, index, futures = job
        images = [f.result() for f in futures]
        host = dict(indices=list(idxs), images=images, epoch=epoch,
                    index=index,
                    filenames=[self.dataset.img_names(i) for i in idxs])
        shapes = [tuple(im.shape[:2]) for im in images]
        if self.test_mode:
            host['plans'] = [self.pipeline.view_plans(s) for s in shapes]
            return host
        rng = np.random if self.seed is None else np.random.RandomState(
            batch_seed(self.seed, epoch, index))
        if self.pipeline.augmented:
            host['plans'] = [self._plan_or_replace(host, k, rng)
                             for k in range(len(images))]
            idxs = host['indices']
        else:
            host['plans'] = self.pipeline.plan(shapes, rng)
        anns = [self.dataset.get_ann_info(i) for i in idxs]
        host['gt_bboxes'] = [a['bboxes'] for a in anns]
        host['gt_labels'] = [a['labels'] for a in anns]
        host['gt_bboxes_ignore'] = [
            a.get('bboxes_ignore', np.zeros((0, 4), np.float32))
            for a in anns]
        return host

    def _plan_or_replace(self, host, k, rng):
        """The plan of image ``k`` of the batch.  A plan the pipeline rejects
        (RandomCrop left no gt box: the reference's pipeline returns None) is
        answered as ``CustomDataset.__getitem__`` answers it (custom.py:
        184-203, ``_rand_another``): another index of the same aspect-ratio
        group, drawn from the batch's generator, decoded here and planned
        again.  ``host`` is updated in place."""
        flag = getattr(self.dataset, 'flag', None)
        for _ in range(MAX_REPLACEMENTS):
            idx = host['indices'][k]
            ann = self.dataset.get_ann_info(idx)
            plan = self.pipeline.plan_image(
                tuple(host['images'][k].shape[:2]), rng, ann['bboxes'],
                ann['labels'], ann.get('bboxes_ignore'))
            if not plan['rejected']:
                return plan
            pool = np.arange(len(self.dataset)) if flag is None else \
                np.where(np.asarray(flag) == flag[idx])[0]
            idx = int(rng.choice(pool))
            host['indices'][k] = idx
            host['images'][k] = self._decode(idx)
            host['filenames'][k] = self.dataset.img_names(idx)
        raise RuntimeError(
            f'no image of the group of index {idx} survives the crop after '
            f'{MAX_REPLACEMENTS} replacements')

    def host_batch(self, epoch, index, order=None):
        """The host half of batch ``index`` of ``epoch``: ``indices``, decoded
        ``images``, ``plans`` (train: one plan per image, drawn from the
        batch's own generator; test: the view plans of every image),
        ``filenames`` and, in train mode, the annotations."""
        if order is None:
            order = self.epoch_order(epoch)
        return self._finish(self._submit(order, epoch, index))

    # -- device half ----------------------------------------------------------
    def device_batch(self, host):
        pipe = self.pipeline
        if not self.test_mode:
            data = pipe(host['images'], host['gt_bboxes'], host['gt_labels'],
                        plans=host['plans'],
                        gt_bboxes_ignore=host['gt_bboxes_ignore'])
            for m, (name, ori) in zip(data['img_metas'], host['filenames']):
                m['filename'], m['ori_filename'] = name, ori
            return data
        if self.multi_view:
            imgs, metas = pipe.aug_views(host['images'][0])
            for view in metas:
                view[0]['filename'], view[0]['ori_filename'] = \
                    host['filenames'][0]
            return dict(img=imgs, img_metas=metas)
        res = pipe(host['images'], plans=[p[0] for p in host['plans']])
        for m, p, (name, ori) in zip(res['img_metas'], host['plans'],
                                     host['filenames']):
            m['flip_direction'] = p[0]['flip_direction']
            m['scale'] = p[0]['scale']
            m['filename'], m['ori_filename'] = name, ori
        return dict(img=[res['img']], img_metas=[res['img_metas']])

    def host_batches(self, epoch=None):
        """The host halves of one epoch in order.  While the caller holds
        batch ``k`` at most the ``LOOK_AHEAD`` batches ``k + 1 .. k +
        LOOK_AHEAD`` have been started: the queue is topped up only when the
        caller comes back for the next one."""
        epoch = self.epoch if epoch is None else int(epoch)
        order = self.epoch_order(epoch)
        n = int(math.ceil(len(order) / self.batch_size))
        jobs, nxt = deque(), 0
        while True:
            # the batch to hand out next and LOOK_AHEAD behind it
            while nxt < n and len(jobs) < LOOK_AHEAD + 1:
                jobs.append(self._submit(order, epoch, nxt))
                nxt += 1
            if not jobs:
                return
            yield self._finish(jobs.popleft())

    def __iter__(self):
        for host in self.host_batches():
            yield self.device_batch(host)

    def __call__(self, epoch):
        """``make_epoch_batches`` of ``EpochRunner.run``."""
        self.set_epoch(epoch)
        return iter(self)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VirtualRankLoader:
    """The loaders of ranks 0 .. W-1 of a W-process job in one process
    (``SGDTrainer(virtual_ranks=W)``): item ``i`` is the list of W device
    batches, the ``r``-th exactly batch ``i`` of ``DeviceDataLoader(dataset,
    samples_per_gpu, ..., dist=True, num_replicas=W, rank=r, seed=seed)`` --
    the same ``DistributedGroupSampler`` order, the same ``(seed, epoch,
    index)`` draws, the same annotations.  ``len()`` is one rank's.

    The W rank loaders share ONE decode pool of ``min(workers_per_gpu * 2,
    16)`` threads (or ``num_threads``), whatever W is, and at most
    ``LOOK_AHEAD`` steps (of W batches each) are started beyond the one
    handed out."""

    def __init__(self, dataset, samples_per_gpu, workers_per_gpu,
                 virtual_ranks, shuffle=True, seed=None, device=None,
                 num_threads=None):
        W = int(virtual_ranks)
        if W < 1:
            raise NotImplementedError(
                f'virtual_ranks={virtual_ranks}: a job has at least one rank')
        if getattr(dataset, 'test_mode', False):
            raise NotImplementedError(
                f'virtual_ranks={W} with a test-mode dataset: virtual ranks '
                'are a train-step notion')
        self.virtual_ranks = W
        self.ranks = [DeviceDataLoader(dataset, samples_per_gpu,
                                       workers_per_gpu, dist=True,
                                       shuffle=shuffle, seed=seed,
                                       device=device, num_replicas=W, rank=r,
                                       num_threads=num_threads)
                      for r in range(W)]
        self.dataset, self.seed = dataset, seed
        self.num_threads = self.ranks[0].num_threads
        self.epoch = 0
        self._pool = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.ranks[0])

    def _share_pool(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.num_threads,
                                            thread_name_prefix='ld-decode')
        for ld in self.ranks:
            ld._pool = self._pool

    def host_batch(self, epoch, index):
        """The W host halves of step ``index`` of ``epoch``, rank 0's first."""
        self._share_pool()
        jobs = [ld._submit(ld.epoch_order(epoch), epoch, index)
                for ld in self.ranks]
        return [ld._finish(j) for ld, j in zip(self.ranks, jobs)]

    def host_batches(self, epoch=None):
        epoch = self.epoch if epoch is None else int(epoch)
        self._share_pool()
        orders = [ld.epoch_order(epoch) for ld in self.ranks]
        n = len(self)
        jobs, nxt = deque(), 0
        while True:
            while nxt < n and len(jobs) < LOOK_AHEAD + 1:
                jobs.append([ld._submit(o, epoch, nxt)
                             for ld, o in zip(self.ranks, orders)])
                nxt += 1
            if not jobs:
                return
            step = jobs.popleft()
            yield [ld._finish(j) for ld, j in zip(self.ranks, step)]

    def device_batch(self, hosts):
        return [ld.device_batch(h) for ld, h in zip(self.ranks, hosts)]

    def __iter__(self):
        for hosts in self.host_batches():
            yield self.device_batch(hosts)

    def __call__(self, epoch):
        self.set_epoch(epoch)
        return iter(self)

    def close(self):
        for ld in self.ranks:
            ld._pool = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_dataloader(dataset, samples_per_gpu, workers_per_gpu, dist=False,
                     shuffle=True, seed=None, device=None, virtual_ranks=None,
                     **kwargs):
    """builder.py:76-140 -> a ``DeviceDataLoader``.  ``num_gpus`` (DataParallel
    batches) is refused: one process drives one device.  ``num_threads=``
    (1 .. 16) sets the decode pool's size directly.  ``virtual_ranks=W`` gives
    a ``VirtualRankLoader``: the W rank-local batches of every step of a
    W-process job."""
    if kwargs.pop('num_gpus', 1) != 1:
        raise NotImplementedError('num_gpus > 1: one process per device')
    if virtual_ranks is not None:
        if dist:
            raise NotImplementedError(
                f'virtual_ranks={virtual_ranks} with dist=True: virtual ranks '
                'composed with real ranks are not implemented')
        return VirtualRankLoader(dataset, samples_per_gpu, workers_per_gpu,
                                 virtual_ranks, shuffle, seed, device,
                                 **kwargs)
    return DeviceDataLoader(dataset, samples_per_gpu, workers_per_gpu, dist,
                            shuffle, seed, device, **kwargs)
