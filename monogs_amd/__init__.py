"""monogs_amd -- MI355X-native differentiable Gaussian rasteriser with camera-pose Jacobians,
a drop-in for MonoGS's ``diff_gaussian_rasterization`` and ``simple_knn``."""
__version__ = "0.1.0"


def __getattr__(name):
    # render_features / FeatureRasterizer (monogs_amd.feature_render) on first use: importing the package stays free of torch
    if name in ("render_features", "FeatureRasterizer"):
        from . import feature_render
        return getattr(feature_render, name)
    # the stereo front end (monogs_amd.stereo) likewise
    if name in ("StereoMatcher", "StereoIngest", "EuRoCParser", "StereoDataset", "load_stereo_dataset", "rectify_map"):
        from . import stereo
        return getattr(stereo, name)
    # the headless viewer (monogs_amd.viewer) likewise
    if name in ("HeadlessViewer", "Snapshot"):
        from . import viewer
        return getattr(viewer, name)
    # learning and scoring the object layer (monogs_amd.object_layer) likewise
    if name in ("LabelTarget", "LabelGrads", "label_loss_grads", "get_loss_labels", "label_confusion", "segmentation_scores",
                "ObjectLayerTrainer", "eval_segmentation", "render_labels"):
        from . import object_layer
        return getattr(object_layer, name)
    # TSDF fusion and mesh extraction (monogs_amd.tsdf) likewise
    if name in ("TSDFVolume", "TriangleMesh", "fuse_map", "mesh_stats", "mesh_from_map"):
        from . import tsdf
        return getattr(tsdf, name)
    # reconstruction evaluation against a ground-truth mesh (monogs_amd.mesh_eval) likewise
    if name in ("nearest_distance", "sample_mesh", "seen_vertices", "cull_mesh", "eval_reconstruction", "recon_metrics"):
        from . import mesh_eval
        return getattr(mesh_eval, name)
    # mesh rendering and Depth L1 (monogs_amd.mesh_render) likewise
    if name in ("MeshRenderer", "render_mesh", "eval_depth_l1", "depth_l1_row"):
        from . import mesh_render
        return getattr(mesh_render, name)
    # median depth, depth variance, depth normals and the geometry figures (monogs_amd.surface) likewise
    if name in ("surface_depth", "depth_normals", "eval_geometry", "SurfaceDepth"):
        from . import surface
        return getattr(surface, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
