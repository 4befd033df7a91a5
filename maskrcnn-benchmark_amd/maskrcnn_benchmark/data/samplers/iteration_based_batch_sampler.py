"""IterationBasedBatchSampler (reference data/samplers/iteration_based_batch_sampler.py): re-iterates a batch sampler
until `num_iterations` batches have been yielded, counting from `start_iter` (a resumed run yields the remainder)."""
from torch.utils.data.sampler import BatchSampler


class IterationBasedBatchSampler(BatchSampler):
    def __init__(self, batch_sampler, num_iterations, start_iter=0):
        self.batch_sampler = batch_sampler
        self.num_iterations = num_iterations
        self.start_iter = start_iter

    def __iter__(self):
        iteration = self.start_iter
        while iteration < self.num_iterations:
            # a DistributedSampler shuffles by epoch: one pass over the wrapped sampler is an epoch
            sampler = getattr(self.batch_sampler, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(iteration)
            for batch in self.batch_sampler:
                if iteration >= self.num_iterations:
                    return
                iteration += 1
                yield batch

    def __len__(self):
        return max(self.num_iterations - self.start_iter, 0)
