"""Dataset catalog (reference config/paths_catalog.py): dataset names -> where their files are.  The data root is
DETOPS_DATA_DIR (default "datasets", as the reference's DATA_DIR); `register` adds a dataset by name."""
import os


class DatasetCatalog(object):
    DATA_DIR = os.environ.get("DETOPS_DATA_DIR", "datasets")
    DATASETS = {
        "coco_2017_train": {"img_dir": "coco/train2017", "ann_file": "coco/annotations/instances_train2017.json"},
        "coco_2017_val": {"img_dir": "coco/val2017", "ann_file": "coco/annotations/instances_val2017.json"},
        "coco_2014_train": {"img_dir": "coco/train2014", "ann_file": "coco/annotations/instances_train2014.json"},
        "coco_2014_val": {"img_dir": "coco/val2014", "ann_file": "coco/annotations/instances_val2014.json"},
        "coco_2014_minival": {"img_dir": "coco/val2014", "ann_file": "coco/annotations/instances_minival2014.json"},
        "coco_2014_valminusminival": {"img_dir": "coco/val2014",
                                      "ann_file": "coco/annotations/instances_valminusminival2014.json"},
        "keypoints_coco_2014_train": {"img_dir": "coco/train2014",
                                      "ann_file": "coco/annotations/person_keypoints_train2014.json"},
        "keypoints_coco_2014_val": {"img_dir": "coco/val2014", "ann_file": "coco/annotations/person_keypoints_val2014.json"},
        "keypoints_coco_2014_minival": {"img_dir": "coco/val2014",
                                        "ann_file": "coco/annotations/person_keypoints_minival2014.json"},
        "keypoints_coco_2014_valminusminival": {"img_dir": "coco/val2014",
                                                "ann_file": "coco/annotations/person_keypoints_valminusminival2014.json"},
        "keypoints_coco_2017_train": {"img_dir": "coco/train2017",
                                      "ann_file": "coco/annotations/person_keypoints_train2017.json"},
        "keypoints_coco_2017_val": {"img_dir": "coco/val2017", "ann_file": "coco/annotations/person_keypoints_val2017.json"},
    }
    # Cityscapes as the reference reads it (data/datasets/cityscapes.py): leftImg8bit/<split>/<city>/*_leftImg8bit.png and
    # gtFine/<split>/<city>/*_polygons.json ("poly") or *_instanceIds.png ("mask"); minival: ten images of val
    CITYSCAPES = {
        "cityscapes_%s_instance_%s" % (mode, name): dict(
            {"img_dir": "cityscapes/leftImg8bit", "ann_dir": "cityscapes/gtFine", "split": split, "mode": mode},
            **({"mini": 10} if name == "minival" else {}))
        for mode in ("poly", "mask") for name, split in (("train", "train"), ("val", "val"), ("minival", "val"))}
    REGISTERED = {}

    @staticmethod
    def register(name, ann_file, root):
        """a COCO-json dataset of the user's (absolute paths, or relative to the working directory)"""
        if name.startswith("synthetic_"):
            raise ValueError("names starting with synthetic_ belong to the synthetic generator")
        DatasetCatalog.REGISTERED[name] = {"ann_file": ann_file, "root": root}

    @staticmethod
    def get(name):
        """-> {"factory": "COCODataset", "args": {"root", "ann_file"}}, or for the cityscapes_{poly,mask}_instance_* names
        {"factory": "CityScapesDataset", "args": {"img_dir", "ann_dir", "split", "mode"[, "mini"]}}"""
        if name in DatasetCatalog.REGISTERED:
            return dict(factory="COCODataset", args=dict(DatasetCatalog.REGISTERED[name]))
        if name in DatasetCatalog.DATASETS:
            attrs = DatasetCatalog.DATASETS[name]
            data_dir = DatasetCatalog.DATA_DIR
            return dict(factory="COCODataset", args=dict(root=os.path.join(data_dir, attrs["img_dir"]),
                                                         ann_file=os.path.join(data_dir, attrs["ann_file"])))
        if name in DatasetCatalog.CITYSCAPES:
            attrs = dict(DatasetCatalog.CITYSCAPES[name])
            attrs["img_dir"] = os.path.join(DatasetCatalog.DATA_DIR, attrs["img_dir"])
            attrs["ann_dir"] = os.path.join(DatasetCatalog.DATA_DIR, attrs["ann_dir"])
            return dict(factory="CityScapesDataset", args=attrs)
        raise RuntimeError("Dataset not available: {}".format(name))
