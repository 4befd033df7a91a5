"""GroupedBatchSampler (reference data/samplers/grouped_batch_sampler.py): mini-batches whose elements share a group
(here: an aspect-ratio bin, so that landscape and portrait images are not padded against each other), in an order as
close to the wrapped sampler's as the grouping allows."""
import torch
from torch.utils.data.sampler import BatchSampler


class GroupedBatchSampler(BatchSampler):
    def __init__(self, sampler, group_ids, batch_size, drop_uneven=False):
        self.sampler = sampler
        self.group_ids = torch.as_tensor(group_ids)
        assert self.group_ids.dim() == 1
        self.batch_size = batch_size
        self.drop_uneven = drop_uneven
        self._batches = None

    def _prepare_batches(self):
        order = [int(i) for i in self.sampler]                 # dataset indices in sampling order
        groups = {}
        for position, index in enumerate(order):
            groups.setdefault(int(self.group_ids[index]), []).append((position, index))
        batches = []
        for members in groups.values():                        # members are in sampling order already
            for s in range(0, len(members), self.batch_size):
                batches.append(members[s:s + self.batch_size])
        batches.sort(key=lambda b: b[0][0])                    # by the position of each batch's first element
        if self.drop_uneven:
            batches = [b for b in batches if len(b) == self.batch_size]
        return [[index for _, index in b] for b in batches]

    def __iter__(self):
        batches = self._batches if self._batches is not None else self._prepare_batches()
        self._batches = None
        return iter(batches)

    def __len__(self):
        if self._batches is None:
            self._batches = self._prepare_batches()            # kept for the next __iter__: one draw of the sampler
        return len(self._batches)
