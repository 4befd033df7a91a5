"""Instance masks of one image (reference structures/segmentation_mask.py).

Two representations behind the reference's wrapper `SegmentationMask(instances, size, mode)` (:444-557):

  mode="mask"  `BinaryMaskList` (reference :30-204): dense [n, H, W] planes, what the synthetic dataset produces by default;
  mode="poly"  `PolygonList` of `PolygonInstance`s (reference :208-475): what COCO-shaped datasets deliver.  The geometry
               (transpose, crop, resize, indexing, the short-polygon filter) is the reference's.  Rasterisation is NOT
               pycocotools (not a dependency here) but the restatement of its polygon-to-RLE routine in include/detops.h,
               on the device (csrc/polygon.hip) or, for host tensors, vectorised numpy (_polygon_cpu.py).

The wrapper's default mode stays "mask" here (the reference's is "poly"): existing callers pass it explicitly.
`convert("poly")` from binary masks needs cv2 in the reference and is not built.
"""
import copy

import torch
from torch.nn.functional import interpolate

FLIP_LEFT_RIGHT = 0
FLIP_TOP_BOTTOM = 1


class BinaryMaskList(object):
    """`masks` [n, H, W] (uint8 or bool or float) for an image of `size` = (W, H)."""

    def __init__(self, masks, size):
        assert isinstance(size, (list, tuple)) and len(size) == 2
        if isinstance(masks, BinaryMaskList):
            masks = masks.masks.clone()
        elif isinstance(masks, (list, tuple)):
            masks = torch.stack(list(masks), dim=0).clone() if len(masks) else torch.empty([0, size[1], size[0]])
        elif not isinstance(masks, torch.Tensor):
            raise RuntimeError("Type of `masks` argument could not be interpreted: %s" % type(masks))
        if masks.dim() == 2:
            masks = masks[None]
        assert masks.dim() == 3
        assert masks.shape[1] == size[1], "%s != %s" % (masks.shape[1], size[1])
        assert masks.shape[2] == size[0], "%s != %s" % (masks.shape[2], size[0])
        self.masks = masks
        self.size = tuple(size)

    def transpose(self, method):
        return BinaryMaskList(self.masks.flip(1 if method == FLIP_TOP_BOTTOM else 2), self.size)

    @staticmethod
    def crop_window(box, width, height):
        """Integer crop window of the reference's `crop` (:111-131): rounded, clamped, >= 1 px."""
        xmin, ymin, xmax, ymax = [round(float(b)) for b in box]
        assert xmin <= xmax and ymin <= ymax, str(box)
        xmin = min(max(xmin, 0), width - 1)
        ymin = min(max(ymin, 0), height - 1)
        xmax = max(min(max(xmax, 0), width), xmin + 1)
        ymax = max(min(max(ymax, 0), height), ymin + 1)
        return xmin, ymin, xmax, ymax

    def crop(self, box):
        xmin, ymin, xmax, ymax = self.crop_window(box, *self.size)
        return BinaryMaskList(self.masks[:, ymin:ymax, xmin:xmax], (xmax - xmin, ymax - ymin))

    def resize(self, size):
        if not isinstance(size, (list, tuple)):
            size = (size, size)
        width, height = map(int, size)
        assert width > 0 and height > 0
        out = interpolate(self.masks[None].float(), size=(height, width), mode="bilinear",
                          align_corners=False)[0].type_as(self.masks)
        return BinaryMaskList(out, (width, height))

    def to(self, *args, **kwargs):
        return BinaryMaskList(self.masks.to(*args, **kwargs), self.size)

    def get_mask_tensor(self):
        return self.masks.squeeze(0) if self.masks.shape[0] == 1 else self.masks

    def __len__(self):
        return len(self.masks)

    def __getitem__(self, index):
        if self.masks.numel() == 0:
            raise RuntimeError("Indexing empty BinaryMaskList")
        return BinaryMaskList(self.masks[index], self.size)

    def __iter__(self):
        return iter(self.masks)

    def __repr__(self):
        return "{}(num_instances={}, image_width={}, image_height={})".format(
            self.__class__.__name__, len(self.masks), self.size[0], self.size[1])


class PolygonInstance(object):
    """The polygons of ONE instance: a list of flat fp32 tensors [x0, y0, x1, y1, ...] (reference :208-345)."""

    def __init__(self, polygons, size):
        if isinstance(polygons, (list, tuple)):
            valid = []
            for p in polygons:
                p = torch.as_tensor(p, dtype=torch.float32)
                if len(p) >= 6:  # 3 * 2 coordinates
                    valid.append(p)
            polygons = valid
        elif isinstance(polygons, PolygonInstance):
            polygons = copy.copy(polygons.polygons)
        else:
            raise RuntimeError("Type of argument `polygons` is not allowed:%s" % (type(polygons)))
        self.polygons = polygons
        self.size = tuple(size)

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        width, height = self.size
        dim, idx = (width, 0) if method == FLIP_LEFT_RIGHT else (height, 1)
        flipped = []
        for poly in self.polygons:
            p = poly.clone()
            p[idx::2] = dim - poly[idx::2] - 1  # TO_REMOVE = 1
            flipped.append(p)
        return PolygonInstance(flipped, size=self.size)

    @staticmethod
    def crop_window(box, width, height):
        """The crop window of the reference's `crop` (:273-290): clamped, >= 1 px, NOT rounded (Python floats)."""
        xmin, ymin, xmax, ymax = map(float, box)
        assert xmin <= xmax and ymin <= ymax, str(box)
        xmin = min(max(xmin, 0), width - 1)
        ymin = min(max(ymin, 0), height - 1)
        xmax = max(min(max(xmax, 0), width), xmin + 1)
        ymax = max(min(max(ymax, 0), height), ymin + 1)
        return xmin, ymin, xmax, ymax

    def crop(self, box):
        assert isinstance(box, (list, tuple, torch.Tensor)), str(type(box))
        xmin, ymin, xmax, ymax = self.crop_window(box, *self.size)
        cropped = []
        for poly in self.polygons:
            p = poly.clone()
            p[0::2] = p[0::2] - xmin
            p[1::2] = p[1::2] - ymin
            cropped.append(p)
        return PolygonInstance(cropped, size=(xmax - xmin, ymax - ymin))

    def resize(self, size):
        try:
            iter(size)
        except TypeError:
            assert isinstance(size, (int, float))
            size = size, size
        ratios = tuple(float(s) / float(s_orig) for s, s_orig in zip(size, self.size))
        if ratios[0] == ratios[1]:
            return PolygonInstance([p * ratios[0] for p in self.polygons], size)
        scaled = []
        for poly in self.polygons:
            p = poly.clone()
            p[0::2] *= ratios[0]
            p[1::2] *= ratios[1]
            scaled.append(p)
        return PolygonInstance(scaled, size=size)

    def convert_to_binarymask(self):
        return PolygonList([self], self.size).convert_to_binarymask().masks[0]

    def __len__(self):
        return len(self.polygons)

    def __repr__(self):
        return "{}(num_groups={}, image_width={}, image_height={})".format(
            self.__class__.__name__, len(self.polygons), self.size[0], self.size[1])


class PackedPolygons(object):
    """Polygons of one or several `PolygonList`s as the three arrays of include/detops.h: verts [V, 2] float32,
    poly_offset [P + 1] int32, inst_offset [G + 1] int32; `inst_base[i]` = global index of list i's first instance.
    The three live in ONE int32 buffer (vertices bit-cast), so that `to(device)` is a single copy."""

    def __init__(self, buffer, V, P, G, inst_base):
        self.buffer, self.V, self.P, self.G, self.inst_base = buffer, V, P, G, list(inst_base)
        self.verts = buffer[:2 * V].view(torch.float32).view(V, 2)
        self.poly_offset = buffer[2 * V:2 * V + P + 1]
        self.inst_offset = buffer[2 * V + P + 1:]
        self._moved = {}

    def to(self, device):
        device = torch.device(device)
        if device == self.buffer.device:
            return self
        key = str(device)
        if key not in self._moved:
            self._moved[key] = PackedPolygons(self.buffer.to(device), self.V, self.P, self.G, self.inst_base)
        return self._moved[key]


class PolygonList(object):
    """The `PolygonInstance`s of all objects of one image (reference :348-475).  Vertices stay on the host; `to(device)`
    records where `convert_to_binarymask` rasterises."""

    def __init__(self, polygons, size, device=None):
        if isinstance(polygons, (list, tuple)):
            if len(polygons) == 0:
                polygons = [[[]]]
            if isinstance(polygons[0], (list, tuple)):
                assert isinstance(polygons[0][0], (list, tuple)), str(type(polygons[0][0]))
            else:
                assert isinstance(polygons[0], PolygonInstance), str(type(polygons[0]))
        elif isinstance(polygons, PolygonList):
            size = polygons.size
            device = polygons.device if device is None else device
            polygons = polygons.polygons
        else:
            raise RuntimeError("Type of argument `polygons` is not allowed:%s" % (type(polygons)))
        assert isinstance(size, (list, tuple)), str(type(size))
        self.polygons = []
        for p in polygons:
            p = PolygonInstance(p, size)
            if len(p) > 0:
                self.polygons.append(p)
        self.size = tuple(size)
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self._packed = None

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        return PolygonList([p.transpose(method) for p in self.polygons], self.size, self.device)

    def crop(self, box):
        w, h = box[2] - box[0], box[3] - box[1]
        return PolygonList([p.crop(box) for p in self.polygons], (w, h), self.device)

    def resize(self, size):
        return PolygonList([p.resize(size) for p in self.polygons], size, self.device)

    def to(self, *args, **kwargs):
        device = kwargs.get("device", args[0] if args else None)
        if not isinstance(device, (str, torch.device)):
            return self
        out = PolygonList(self.polygons, self.size, device)
        out._packed = self._packed
        return out

    def packed(self):
        """This list's `PackedPolygons` (host), built once and kept."""
        if self._packed is None:
            self._packed = self.pack([self])
        return self._packed

    @staticmethod
    def pack(lists):
        """Several lists (the images of a batch, in order) as one `PackedPolygons` on the host: the per-list arrays are
        cached on the lists, so the per-step work is a few concatenations."""
        if len(lists) == 1 and lists[0]._packed is None:
            # an odd trailing number is not a vertex
            polys = [p[:len(p) // 2 * 2] for inst in lists[0].polygons for p in inst.polygons]
            verts = torch.cat(polys) if polys else torch.zeros(0)
            poly_offset = [0]
            for p in polys:
                poly_offset.append(poly_offset[-1] + len(p) // 2)
            inst_offset = [0]
            for inst in lists[0].polygons:
                inst_offset.append(inst_offset[-1] + len(inst.polygons))
            buf = torch.cat([verts.to(torch.float32).contiguous().view(torch.int32),
                             torch.tensor(poly_offset, dtype=torch.int32), torch.tensor(inst_offset, dtype=torch.int32)])
            return PackedPolygons(buf, poly_offset[-1], len(polys), len(lists[0].polygons), [0])
        parts = [x.packed() for x in lists]
        if len(parts) == 1:
            return parts[0]
        V = P = G = 0
        verts, poly_offset, inst_offset, base = [], [torch.zeros(1, dtype=torch.int32)], [torch.zeros(1, dtype=torch.int32)], []
        for k in parts:
            base.append(G)
            verts.append(k.buffer[:2 * k.V])
            poly_offset.append(k.poly_offset[1:] + V)
            inst_offset.append(k.inst_offset[1:] + P)
            V, P, G = V + k.V, P + k.P, G + k.G
        return PackedPolygons(torch.cat(verts + poly_offset + inst_offset), V, P, G, base)

    def convert_to_binarymask(self):
        from maskrcnn_benchmark import _C

        width, height = self.size
        assert int(width) == width and int(height) == height, "a dense mask needs an integer image size: %s" % (self.size,)
        k = self.packed().to(self.device)
        masks = _C.polygons_to_masks(k.verts, k.poly_offset, k.inst_offset, int(height), int(width))
        return BinaryMaskList(masks, size=(int(width), int(height)))

    def __len__(self):
        return len(self.polygons)

    def __getitem__(self, item):
        if isinstance(item, int):
            selected = [self.polygons[item]]
        elif isinstance(item, slice):
            selected = self.polygons[item]
        else:
            # advanced indexing on a single dimension
            selected = []
            if isinstance(item, torch.Tensor) and item.dtype in (torch.bool, torch.uint8):
                item = item.nonzero()
                item = item.squeeze(1) if item.numel() > 0 else item
            if isinstance(item, torch.Tensor):
                item = item.tolist()
            for i in item:
                selected.append(self.polygons[i])
        return PolygonList(selected, self.size, self.device)

    def __iter__(self):
        return iter(self.polygons)

    def __repr__(self):
        return "{}(num_instances={}, image_width={}, image_height={})".format(
            self.__class__.__name__, len(self.polygons), self.size[0], self.size[1])


class SegmentationMask(object):
    def __init__(self, instances, size, mode="mask"):
        assert isinstance(size, (list, tuple)) and len(size) == 2
        if isinstance(size[0], torch.Tensor):
            size = size[0].item(), size[1].item()
        if mode == "poly":
            self.instances = instances if isinstance(instances, PolygonList) else PolygonList(instances, size)
        elif mode == "mask":
            self.instances = instances if isinstance(instances, BinaryMaskList) else BinaryMaskList(instances, size)
        else:
            raise NotImplementedError("Unknown mode: %s" % str(mode))
        self.size = tuple(size)
        self.mode = mode

    def transpose(self, method):
        return SegmentationMask(self.instances.transpose(method), self.size, self.mode)

    def crop(self, box):
        c = self.instances.crop(box)
        return SegmentationMask(c, c.size, self.mode)

    def resize(self, size, *args, **kwargs):
        r = self.instances.resize(size)
        return SegmentationMask(r, r.size, self.mode)

    def to(self, *args, **kwargs):
        return SegmentationMask(self.instances.to(*args, **kwargs), self.size, self.mode)

    def convert(self, mode):
        if mode == self.mode:
            return self
        if mode == "mask":
            return SegmentationMask(self.instances.convert_to_binarymask(), self.size, mode)
        if mode == "poly":
            raise NotImplementedError("binary masks to polygons is not built (the reference needs cv2 for it)")
        raise NotImplementedError("Unknown mode: %s" % str(mode))

    def get_mask_tensor(self):
        instances = self.instances.convert_to_binarymask() if self.mode == "poly" else self.instances
        return instances.get_mask_tensor()

    def __len__(self):
        return len(self.instances)

    def __getitem__(self, item):
        return SegmentationMask(self.instances[item], self.size, self.mode)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i:i + 1]

    def __repr__(self):
        return "{}(num_instances={}, image_width={}, image_height={}, mode={})".format(
            self.__class__.__name__, len(self.instances), self.size[0], self.size[1], self.mode)
