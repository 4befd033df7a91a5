"""make_data_loader (reference data/build.py).  Dataset names that start with `synthetic_` (and an empty list) go to the
synthetic generator of data/synthetic.py unchanged; every other name is looked up in the catalog and read as COCO json,
or, for the cityscapes_{poly,mask}_instance_* names, by data/datasets/cityscapes.py.

The real-data loader: an aspect-ratio GroupedBatchSampler under DATALOADER.ASPECT_RATIO_GROUPING, an
IterationBasedBatchSampler of MAX_ITER batches for training, torch's DistributedSampler when distributed, and the
collator of the chosen input path (data/collate_batch.py: DETOPS_INPUT_PREP)."""
import bisect
import copy

import torch
import torch.utils.data

from maskrcnn_benchmark.config.paths_catalog import DatasetCatalog
from maskrcnn_benchmark.utils.comm import get_world_size

from . import collate_batch, samplers, synthetic
from . import datasets as D
from .transforms import build_transforms, jitter_enabled


def _is_synthetic(names):
    return all(n.startswith("synthetic_") for n in names)


def build_dataset(dataset_list, transforms, dataset_catalog, is_train=True):
    """-> [dataset] (training: one ConcatDataset when several are named)"""
    if not isinstance(dataset_list, (list, tuple)):
        raise RuntimeError("dataset_list should be a list of strings, got {}".format(dataset_list))
    out = []
    for name in dataset_list:
        data = dataset_catalog.get(name)
        factory = getattr(D, data["factory"])
        args = dict(data["args"])
        args["remove_images_without_annotations"] = is_train
        args["transforms"] = transforms
        dataset = factory(**args)
        dataset.groundtruth_targets = not is_train
        out.append(dataset)
    if is_train and len(out) > 1:
        return [ConcatDataset(out)]
    return out


class ConcatDataset(torch.utils.data.ConcatDataset):
    """torch's, with get_img_info routed to the member (the reference's data/datasets/concat_dataset.py)"""

    def get_idxs(self, idx):
        d = bisect.bisect_right(self.cumulative_sizes, idx)
        return d, idx if d == 0 else idx - self.cumulative_sizes[d - 1]

    def get_img_info(self, idx):
        d, i = self.get_idxs(idx)
        return self.datasets[d].get_img_info(i)


def make_data_sampler(dataset, shuffle, distributed):
    if distributed:
        return torch.utils.data.distributed.DistributedSampler(dataset, shuffle=shuffle)
    if shuffle:
        return torch.utils.data.sampler.RandomSampler(dataset)
    return torch.utils.data.sampler.SequentialSampler(dataset)


def _quantize(x, bins):
    bins = sorted(copy.copy(bins))
    return [bisect.bisect_right(bins, y) for y in x]


def _compute_aspect_ratios(dataset):
    ratios = []
    for i in range(len(dataset)):
        info = dataset.get_img_info(i)
        ratios.append(float(info["height"]) / float(info["width"]))
    return ratios


def make_batch_data_sampler(dataset, sampler, aspect_grouping, images_per_batch, num_iters=None, start_iter=0):
    if aspect_grouping:
        if not isinstance(aspect_grouping, (list, tuple)):
            aspect_grouping = [aspect_grouping]
        group_ids = _quantize(_compute_aspect_ratios(dataset), aspect_grouping)
        batch_sampler = samplers.GroupedBatchSampler(sampler, group_ids, images_per_batch, drop_uneven=False)
    else:
        batch_sampler = torch.utils.data.sampler.BatchSampler(sampler, images_per_batch, drop_last=False)
    if num_iters is not None:
        batch_sampler = samplers.IterationBasedBatchSampler(batch_sampler, num_iters, start_iter)
    return batch_sampler


def deferred_prep(cfg, is_train):
    """are the pixels of this loader's batches deferred (ToRaw transforms, RawBatchCollator)?  The input path's switch
    (collate_batch.device_prep), and always under test-time box augmentation: every pass is prepared from the raw bytes;
    and always for a training loader with non-zero colour jitter, which only the deferred path serves (on a GPU and on the
    CPU alike)."""
    return collate_batch.device_prep(cfg) or (not is_train and cfg.TEST.BBOX_AUG.ENABLED) or jitter_enabled(cfg, is_train)


def make_collator(cfg, is_train=True):
    if deferred_prep(cfg, is_train):
        from maskrcnn_benchmark.engine.bench_step import choose_layout

        return collate_batch.RawBatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD,
                                              cfg.INPUT.TO_BGR255, choose_layout(cfg, cfg.MODEL.DEVICE) != "nchw")
    return collate_batch.BatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY)


def make_data_loader(cfg, is_train=True, is_distributed=False, start_iter=0, images_per_gpu=None, length=None,
                     dataset_name=None):
    """-> ONE loader, as the synthetic function returns and tools/test_net.py expects: training, the remaining iterations
    over DATASETS.TRAIN (several names are concatenated); testing, the dataset `dataset_name` of DATASETS.TEST, which may
    be left out when DATASETS.TEST names one dataset.  (The reference returns a list of test loaders; a caller that wants
    one per name asks for each by name.)"""
    names = cfg.DATASETS.TRAIN if is_train else cfg.DATASETS.TEST
    if _is_synthetic(names):
        if not is_train and cfg.TEST.BBOX_AUG.ENABLED:
            raise ValueError("TEST.BBOX_AUG prepares every pass from the raw uint8 images (the deferred input path); the "
                             "synthetic generator %s makes float tensors: name a COCO-json dataset in DATASETS.TEST"
                             % (tuple(names),))
        return synthetic.make_data_loader(cfg, is_train=is_train, is_distributed=is_distributed, start_iter=start_iter,
                                          images_per_gpu=images_per_gpu, length=length)
    if not is_train:
        if dataset_name is None and len(names) != 1:
            raise ValueError("DATASETS.TEST names %d datasets: ask for one with dataset_name=" % len(names))
        if dataset_name is not None and dataset_name not in names:
            raise ValueError("%r is not in DATASETS.TEST %s" % (dataset_name, tuple(names)))
        names = (names[0] if dataset_name is None else dataset_name,)
    world = get_world_size()
    if images_per_gpu is None:
        total = cfg.SOLVER.IMS_PER_BATCH if is_train else cfg.TEST.IMS_PER_BATCH
        assert total % world == 0, "IMS_PER_BATCH ({}) must be divisible by the number of GPUs ({})".format(total, world)
        images_per_gpu = total // world
    shuffle = is_train
    num_iters = cfg.SOLVER.MAX_ITER if is_train else None
    if not is_train:
        start_iter = 0
    aspect_grouping = [1] if cfg.DATALOADER.ASPECT_RATIO_GROUPING else []
    deferred = deferred_prep(cfg, is_train)
    transforms = build_transforms(cfg, is_train, device_prep=deferred)
    loaders = []
    for dataset in build_dataset(names, transforms, DatasetCatalog, is_train):
        sampler = make_data_sampler(dataset, shuffle, is_distributed)
        batch_sampler = make_batch_data_sampler(dataset, sampler, aspect_grouping, images_per_gpu, num_iters, start_iter)
        loaders.append(torch.utils.data.DataLoader(dataset, num_workers=cfg.DATALOADER.NUM_WORKERS, batch_sampler=batch_sampler,
                                                   collate_fn=make_collator(cfg, is_train),
                                                   pin_memory=cfg.MODEL.DEVICE != "cpu" and deferred))
    assert len(loaders) == 1
    return loaders[0]
