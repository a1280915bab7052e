"""What blend_backward_s_kernel fetches now that it walks the forward's survivor masks, against what its own cull kept
(mgs_debug_blend_mask_stats), at C5 and at 100 k / VGA.  An extra survivor has no active pixel and costs ~29 vector instructions
and a record fetch; the cull that is gone cost ~120 per 64-instance step: break-even ~4 extra per step."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from monogs_amd.rasterizer import (GaussianRasterizationSettings, GaussianRasterizer,  # noqa: E402
                                   debug_blend_mask_stats)
from monogs_amd.synthetic import make_scene, scene_settings  # noqa: E402

DEV = "cuda:0"
for P, intr in ((2000000, "davis_1080p"), (100000, "fr3_office")):
    sc = make_scene(P, intr, seed=1)
    st = scene_settings(sc, GaussianRasterizationSettings, device=DEV)
    d = lambda x: x.to(DEV)  # noqa: E731
    means = d(sc.means3D).requires_grad_(True)
    out = GaussianRasterizer(st)(means3D=means, means2D=torch.zeros_like(means), opacities=d(sc.opacities),
                                 colors_precomp=d(sc.colors), scales=d(sc.scales.repeat(1, 3)), rotations=d(sc.rotations))
    s = debug_blend_mask_stats(out[0])
    extra = s["forward_masks"] - s["own_cull"]
    print(f"{P} {intr}: steps {s['steps']}, survivors of the backward's own cull {s['own_cull']} ({s['own_cull'] / s['steps']:.2f} per step), "
          f"set bits of the forward's masks {s['forward_masks']} (+{extra}, {100.0 * extra / s['own_cull']:.2f} %, "
          f"{extra / s['steps']:.2f} per step), kept by the own cull and missing in the mask {s['missing']}")
