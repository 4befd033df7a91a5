"""Instance masks of one image as uncompressed COCO RLE: what a `segm.json` result file, a crowd annotation, or
`_C.paste_masks_rle` holds.  A BoxList field (`mask` of a prediction, `masks` of a target) that the evaluator packs into
bit rows with `_C.mask_pack_rle` without ever laying out a plane.

counts int32 [total] and run_offset int64 [N + 1]: mask n's run lengths, column-major and starting with a 0-run, are
counts[run_offset[n]:run_offset[n + 1]].  size = (width, height) of the image, as BoxList.size.
"""
import torch

from maskrcnn_benchmark import _C


class RLEMasks(object):
    def __init__(self, counts, run_offset, size):
        counts, run_offset = torch.as_tensor(counts), torch.as_tensor(run_offset)
        if counts.dtype != torch.int32 or run_offset.dtype != torch.int64 or counts.dim() != 1 or run_offset.dim() != 1 \
                or run_offset.numel() < 1 or counts.device != run_offset.device:
            raise ValueError("RLEMasks: expected counts int32 [total] and run_offset int64 [N + 1] on one device")
        self.counts, self.run_offset = counts, run_offset
        self.size = (int(size[0]), int(size[1]))

    @classmethod
    def from_strings(cls, strings, size, device=None):
        """compressed `counts` strings of masks of one image; malformed strings, and runs that do not sum to the image's
        height * width, raise ValueError"""
        W, H = int(size[0]), int(size[1])
        strings = list(strings)
        counts, run_offset = _C.rle_string_decode_list(strings, [(H, W)] * len(strings), device)
        return cls(counts, run_offset, (W, H))

    @classmethod
    def from_lists(cls, lists, size, device=None):
        """uncompressed `counts` lists of masks of one image"""
        W, H = int(size[0]), int(size[1])
        lengths = torch.tensor([len(c) for c in lists], dtype=torch.int64)
        for n, c in enumerate(lists):
            if min(c, default=0) < 0 or sum(c) != H * W:
                raise ValueError("RLEMasks: the runs of mask %d do not cover the %d x %d image" % (n, H, W))
        counts = torch.tensor([v for c in lists for v in c], dtype=torch.int32)
        run_offset = torch.cat([lengths.new_zeros(1), torch.cumsum(lengths, 0)])
        out = cls(counts, run_offset, (W, H))
        return out if device is None else out.to(device)

    @property
    def device(self):
        return self.counts.device

    def __len__(self):
        return self.run_offset.numel() - 1

    def hw(self):
        """-> [(H, W)] * N, the `hw` of _C.mask_pack_rle"""
        return [(self.size[1], self.size[0])] * len(self)

    def to(self, device):
        return RLEMasks(self.counts.to(device), self.run_offset.to(device), self.size)

    def resize(self, size, *args, **kwargs):
        """runs cannot be rescaled: only the mask's own size is served"""
        if (int(size[0]), int(size[1])) != self.size:
            raise ValueError("RLEMasks of an image of %s cannot be resized to %s" % (self.size, tuple(size)))
        return self

    def __getitem__(self, item):
        """an int, a slice, or an index / bool tensor, as BoxList indexes its fields"""
        if isinstance(item, int):
            item = [item]
        index = torch.arange(len(self), device=self.device)[item].reshape(-1)
        ro = self.run_offset
        lengths = (ro[1:] - ro[:-1])[index]
        new_offset = torch.cat([lengths.new_zeros(1), torch.cumsum(lengths, 0)])
        which = torch.repeat_interleave(torch.arange(index.numel(), device=self.device), lengths)
        pos = torch.arange(int(new_offset[-1]), device=self.device) - new_offset[:-1][which] + ro[:-1][index][which]
        return RLEMasks(self.counts[pos], new_offset, self.size)

    def __repr__(self):
        return "RLEMasks(num_masks=%d, image_width=%d, image_height=%d)" % (len(self), self.size[0], self.size[1])
