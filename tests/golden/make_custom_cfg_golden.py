#!/usr/bin/env python3
"""Generates tests/golden/custom_data_model_cfg.json: the merged `model` dict of the reference's custom_data configs
(projects/BEVFusion/configs/custom_data/lidar-cam_custom.py over its base lidar_custom.py).  Run in the build container
only (needs the reference checkout, REFERENCE_ROOT or /root/reference); the test-suite reads the committed .json.

The two files are mmengine configs: plain Python whose module-level names are the settings.  mmengine is not installed
here, so its `_base_` rule is restated: every base file is evaluated first, the child sees the base's names as
attributes of `_base_` (`_base_.point_load_dim`, `del _base_.custom_hooks`), and a dict of the child is merged
RECURSIVELY over the dict of the same name in the base (a non-dict value replaces).  Only the resulting `model` dict is
stored: settings, no code.
"""
import ast
import json
import os
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
CHILD = os.path.join(REF, "projects", "BEVFusion", "configs", "custom_data", "lidar-cam_custom.py")
OUT = os.path.join(HERE, "custom_data_model_cfg.json")


def merge(base, child):
    out = dict(base)
    for k, v in child.items():
        out[k] = merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def load(path):
    """-> dict of the file's settings with its bases merged underneath."""
    with open(path, encoding="utf-8") as f:
        tree = ast.parse(f.read(), path)
    bases, body = [], []
    for node in tree.body:
        if (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
                and node.targets[0].id == "_base_"):
            val = ast.literal_eval(node.value)
            bases = [val] if isinstance(val, str) else list(val)
        else:
            body.append(node)
    merged = {}
    for b in bases:
        merged = merge(merged, load(os.path.normpath(os.path.join(os.path.dirname(path), b))))
    base_ns = types.SimpleNamespace(**merged)
    scope = {"_base_": base_ns}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), scope)
    own = {k: v for k, v in scope.items() if k not in ("_base_", "__builtins__") and not isinstance(v, types.ModuleType)}
    # names the child deleted from `_base_` are gone from the result as well
    return merge({k: v for k, v in merged.items() if hasattr(base_ns, k)}, own)


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


if __name__ == "__main__":
    model = plain(load(CHILD)["model"])
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(model, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "-", len(json.dumps(model)), "bytes")
