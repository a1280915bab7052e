"""Which module depends on which: the product modules (frame types, tracker, sequences, dataset readers) stand on their own and
``monogs_amd.slam_harness`` -- the two run loops that measure them -- sits on top, imported by nothing in the package."""
import ast
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "monogs_amd")


def _imported_names(tree):
    """Every dotted module name and imported name an import statement of ``tree`` mentions, at any depth."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            yield from (a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            yield node.module or ""
            yield from (a.name for a in node.names)


def test_only_the_harness_imports_the_harness():
    paths = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(paths) > 20
    for path in paths:
        if os.path.basename(path) == "slam_harness.py":
            continue
        with open(path) as f:
            names = list(_imported_names(ast.parse(f.read())))
        assert not [n for n in names if "slam_harness" in n.split(".")], path


def test_the_harness_defines_only_private_classes():
    with open(os.path.join(PKG, "slam_harness.py")) as f:
        classes = [n.name for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.ClassDef)]
    assert all(c.startswith("_") for c in classes), classes


def test_names_live_in_their_modules():
    from monogs_amd.eager_probe import eager_tracking_probe, reference_style_tracking_loss
    from monogs_amd.frames import Intrinsics, Viewpoint, position_error, scharr_grad_mask
    from monogs_amd.sequences import ROOM_SURFACES, make_room_sequence, make_sequence, raycast_room
    from monogs_amd.slam_harness import make_sequence as reexported, run_slam, run_slam_two_process
    from monogs_amd.tracking import TrackingGraph, track_eager
    for obj, module in ((Intrinsics, "frames"), (Viewpoint, "frames"), (position_error, "frames"), (scharr_grad_mask, "frames"),
                        (TrackingGraph, "tracking"), (track_eager, "tracking"), (make_sequence, "sequences"),
                        (make_room_sequence, "sequences"), (raycast_room, "sequences"), (eager_tracking_probe, "eager_probe"),
                        (reference_style_tracking_loss, "eager_probe"), (run_slam, "slam_harness"),
                        (run_slam_two_process, "slam_harness")):
        assert obj.__module__ == "monogs_amd." + module, (obj, obj.__module__)
    assert reexported is make_sequence and ROOM_SURFACES == 18


def test_the_map_step_has_one_home():
    """The activations, their backward and the schedule step are each launched from ONE place; the window mapper and the refiner
    reach them through ``map_step`` and name none of them; what only renders the map does not import the window mapper."""
    symbols = ("mgs_activate_forward", "mgs_activate_backward", "mgs_lr_schedule_step")
    calls = {s: [] for s in symbols}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in calls:
                calls[node.func.attr].append((os.path.basename(path), node.lineno))
    assert all(len(v) == 1 for v in calls.values()), calls
    for name in ("mapping.py", "refinement.py"):
        with open(os.path.join(PKG, name)) as f:
            text = f.read()
        assert not [s for s in symbols if s in text], name
    for name in ("tracking.py", "sequences.py"):
        with open(os.path.join(PKG, name)) as f:
            names = list(_imported_names(ast.parse(f.read())))
        assert not [n for n in names if "mapping" in n.split(".")], name
    import monogs_amd.map_step
    import monogs_amd.mapping
    assert monogs_amd.mapping.render_map is monogs_amd.map_step.render_map


def test_the_dataset_readers_do_not_load_the_harness():
    code = ("import sys; import monogs_amd.dataset, monogs_amd.frame_ingest, monogs_amd.renderer; "
            "sys.exit(1 if 'monogs_amd.slam_harness' in sys.modules else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_call_helpers_live_in_launch():
    """``_stream``, ``_device_guard``, ``_ptr`` and ``_f32`` have nothing to do with rasterisation: every module takes them from
    ``_launch``; only ``rasterizer`` itself names them (it re-exports them for tests and tools)."""
    helpers = {"_stream", "_device_guard", "_ptr", "_f32"}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        if os.path.basename(path) == "rasterizer.py":
            continue
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[-1] == "rasterizer":
                assert not helpers & {a.name for a in node.names}, (path, node.lineno)
    import monogs_amd._launch
    import monogs_amd.rasterizer
    for name in sorted(helpers | {"_raw_stream"}):
        assert getattr(monogs_amd.rasterizer, name) is getattr(monogs_amd._launch, name), name
    assert monogs_amd.rasterizer._camera.__module__ == "monogs_amd.rasterizer"


def test_the_binding_does_not_import_torch():
    for name in ("_lib.py", "_header.py"):
        with open(os.path.join(PKG, name)) as f:
            names = list(_imported_names(ast.parse(f.read())))
        assert not [n for n in names if n.split(".")[0] == "torch"], name


def test_knn_does_not_load_the_rasteriser():
    code = "import sys; import monogs_amd.knn; sys.exit(1 if 'monogs_amd.rasterizer' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
