"""Generate tests/golden/whole_model_mask_rcnn_gn.npz: the GroupNorm Mask R-CNN of the reference
(configs/gn_baselines/e2e_mask_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml), built narrow by the machinery of
make_golden_whole_model.py (same stand-ins, same batch, same seeds) — see that file for what the fixture pins and how the
reference is made importable.  tests/test_group_norm_cpu.py and tests/test_group_norm_model_gpu.py load it.

Two things differ from the FrozenBN case.  The narrow widths need narrow groups: MODEL.GROUP_NORM.NUM_GROUPS -1 with
DIM_PER_GP 2 (every width here is even), and the conv box head gets CONV_HEAD_DIM 16.  And the reference's `group_norm()`
(modeling/make_layers.py:24-39) reads its GLOBAL cfg, not the clone the model is built from, so the two GROUP_NORM keys are
merged into the global as well.  This repository's builders take them from the cfg they are given.

Run:  python tests/golden/make_golden_whole_model_gn.py      (build container only)
"""
import make_golden_whole_model as base

GROUP_NORM = ["MODEL.GROUP_NORM.NUM_GROUPS", -1, "MODEL.GROUP_NORM.DIM_PER_GP", 2]
base.CASES["mask_rcnn_gn"] = ("gn_baselines/e2e_mask_rcnn_R_50_FPN_Xconv1fc_1x_gn.yaml",
                              base.CASES["mask_rcnn"][1] + GROUP_NORM + ["MODEL.ROI_BOX_HEAD.CONV_HEAD_DIM", 16])

if __name__ == "__main__":
    base.ref_cfg.merge_from_list(GROUP_NORM)
    base.run("mask_rcnn_gn")
