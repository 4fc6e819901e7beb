"""Plug-in registration under the reference's registry names.

The reference finds its modules by NAME through mmengine's registry
(`@MODELS.register_module()`, mmdet3d/registry.py:71-72; names used by the BEVFusion configs:
'DepthLSSTransform', 'LSSTransform', 'BEVFusionSparseEncoder', 'SubMConv3d', 'SparseConv3d', ...).
mmengine/mmdet3d are not installed in this image, so a minimal registry with the same two calls
(`register_module`, `build`) lives here; `register(target)` re-registers every class into a real
mmengine registry (e.g. mmdet3d.registry.MODELS) when one is available -- that one call is the
whole integration on the reference side.
"""


class Registry:
    def __init__(self, name):
        self.name = name
        self._modules = {}

    def register_module(self, name=None, force=False, module=None):
        def _do(cls):
            key = name or cls.__name__
            if key in self._modules and not force and self._modules[key] is not cls:
                raise KeyError("%s is already registered in %s" % (key, self.name))
            self._modules[key] = cls
            return cls
        if module is not None:
            return _do(module)
        return _do

    def get(self, key):
        return self._modules.get(key)

    def build(self, cfg, *args, **kwargs):
        cfg = dict(cfg)
        typ = cfg.pop("type")
        cls = self._modules[typ] if isinstance(typ, str) else typ
        return cls(*args, **cfg, **kwargs)

    def __contains__(self, key):
        return key in self._modules

    def names(self):
        return sorted(self._modules)


MODELS = Registry("models")
# data pipeline steps (mmdet3d.registry.TRANSFORMS): ImageAug3D and GridMask (image_aug.py) and the LiDAR chain (points_aug.py):
# BEVFusionGlobalRotScaleTrans, GlobalRotScaleTrans, BEVFusionRandomFlip3D, PointsRangeFilter, ObjectRangeFilter,
# ObjectNameFilter, PointShuffle; ObjectSample and its DataBaseSampler (object_sample.py); LoadPointsFromFile,
# LoadPointsFromMultiSweeps, LoadAnnotations3D and BEVLoadMultiViewImageFromFiles (loading.py).  gt_database.py builds the
# database DataBaseSampler reads with the first three of those.
TRANSFORMS = Registry("transforms")
# evaluators (mmdet3d.registry.METRICS): NuScenesCustomMetric (evaluation.py), the `val_evaluator` of the reference's custom-data
# configs -- the nuScenes detection protocol (matching, PR curves, mAP, the TP errors, NDS) on what predict() returns.
METRICS = Registry("metrics")
# what draws predictions (mmdet3d.registry.VISUALIZERS): PredictionVisualizer (visualize.py), the reference's two tools/visualize
# scripts as one callable -- not mmengine's Det3DLocalVisualizer interface.
VISUALIZERS = Registry("visualizers")


def register(target):
    """Register every class of this package into `target` (an mmengine Registry) under the
    reference's names, overriding the CUDA-backed originals."""
    for key, cls in MODELS._modules.items():
        target.register_module(name=key, force=True, module=cls)
    return target
