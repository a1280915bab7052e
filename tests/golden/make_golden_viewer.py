"""Records ``jet_lut.npy``: matplotlib's "jet" as the reference's viewer uses it (viewer/slam_viewer.py:614-618, :628-632:
``color_map(x)[..., :3] * 255`` cast to bytes), one row per table entry.  Needs matplotlib (3.10.8 wrote the committed file); the
tests read the file only.
  python tests/golden/make_golden_viewer.py"""
import os

import numpy as np


def main():
    import matplotlib
    cmap = matplotlib.colormaps.get_cmap("jet")
    assert cmap.N == 256
    lut = (cmap(np.arange(256))[:, :3] * 255).astype(np.uint8)
    # the same entries through the float path the reference takes: x -> int(x * 256)
    x = ((np.arange(256) + 0.5) / 256).astype(np.float32)
    assert np.array_equal((cmap(x)[..., :3] * 255).astype(np.uint8), lut)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jet_lut.npy")
    np.save(out, lut)
    print("wrote", out, lut.shape, lut.dtype, "matplotlib", matplotlib.__version__)


if __name__ == "__main__":
    main()
