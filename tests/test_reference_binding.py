"""The reference's OWN render seam binds to the drop-in packages: `gaussian_splatting/gaussian_renderer/__init__.py`
imports `diff_gaussian_rasterization` (:13-16), builds the settings tuple by keyword (:70-84) and calls the rasteriser by
keyword (:145-156).  Its imports and call sites were read with `ast` into tests/golden/render_seam.json
(tests/golden/make_golden.py::render_seam); nothing is executed on a GPU here."""
import inspect
import json
import os

SEAM = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_seam.json")))


def test_reference_render_seam_binds_to_the_shim():
    import diff_gaussian_rasterization as shim
    from monogs_amd import rasterizer
    seam = SEAM["renderer"]
    names = seam["imports_diff_gaussian_rasterization"]
    assert {"GaussianRasterizer", "GaussianRasterizationSettings"} <= set(names)
    for name in names:                   # every name the seam imports resolves to ours
        assert getattr(shim, name) is getattr(rasterizer, name), name
    assert "render" in seam["functions"]

    # settings: every keyword the reference passes is a field, and every field is passed
    (call,) = seam["settings_calls"]
    assert call["n_args"] == 0 and sorted(call["keywords"]) == sorted(rasterizer.GaussianRasterizationSettings._fields)
    # rasteriser: the reference's keyword calls are accepted by forward()
    params = set(inspect.signature(rasterizer.GaussianRasterizer.forward).parameters) - {"self"}
    calls = seam["rasterizer_calls"]
    assert calls
    for c in calls:
        assert c["n_args"] == 0 and set(c["keywords"]) <= params, c["keywords"]
    assert {"theta", "rho", "means2D", "colors_precomp", "scales", "rotations"} <= {k for c in calls for k in c["keywords"]}


def test_reference_simple_knn_call_site_binds():
    """`from simple_knn._C import distCUDA2` (the reference's gaussian_splatting/scene/gaussian_model.py:18), called with
    one positional tensor (:294-302)."""
    from simple_knn._C import distCUDA2
    from monogs_amd.knn import distCUDA2 as ours
    assert distCUDA2 is ours
    model = SEAM["gaussian_model"]
    assert "distCUDA2" in model["imports_simple_knn._C"]
    (call,) = model["distCUDA2_calls"]
    assert call["n_args"] == 1 and not call["keywords"]
