"""Writes tests/golden/ssim_seam.json: how the reference reaches ``fused_ssim`` -- read with ``ast`` from
gaussian_splatting/utils/loss_utils.py (the import and the ``fused_ssim(...)`` call inside ``ssim``), utils/slam_mapper.py and
utils/eval_utils.py (the import of ``ssim`` and its call sites) and the ``lambda_ssim`` values of the configs.  Names and
counts only.  Usage: python tests/golden/make_golden_ssim.py [reference root]"""
import ast
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MONOGS_REFERENCE", "/root/reference")


def _calls(tree, name):
    return [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == name]


def _site(c):
    return {"n_args": len(c.args),
            "keywords": {k.arg: (k.value.value if isinstance(k.value, ast.Constant) else None) for k in c.keywords}}


def _imports(tree, module):
    return sorted(a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module == module for a in n.names)


def main():
    parse = lambda *p: ast.parse(open(os.path.join(REF, *p)).read())  # noqa: E731
    loss_utils = parse("gaussian_splatting", "utils", "loss_utils.py")
    out = {"loss_utils": {"imports_fused_ssim": _imports(loss_utils, "fused_ssim"),
                          "module_level_import": any(isinstance(n, ast.ImportFrom) and n.module == "fused_ssim"
                                                     for n in loss_utils.body),
                          "fused_ssim_calls": [_site(c) for c in _calls(loss_utils, "fused_ssim")],
                          "ssim_params": [[a.arg for a in n.args.args] for n in loss_utils.body
                                          if isinstance(n, ast.FunctionDef) and n.name == "ssim"]}}
    for key, path in (("slam_mapper", ("utils", "slam_mapper.py")), ("eval_utils", ("utils", "eval_utils.py"))):
        tree = parse(*path)
        out[key] = {"imports_loss_utils": _imports(tree, "gaussian_splatting.utils.loss_utils"),
                    "ssim_calls": [_site(c) for c in _calls(tree, "ssim")]}
    lambdas = {}
    for cfg in sorted(glob.glob(os.path.join(REF, "configs", "**", "*.yaml"), recursive=True)):
        m = re.search(r"^\s*lambda_ssim:\s*([0-9.eE+-]+)\s*$", open(cfg).read(), flags=re.M)
        if m:
            lambdas[os.path.relpath(cfg, os.path.join(REF, "configs"))] = float(m.group(1))
    out["lambda_ssim"] = lambdas
    with open(os.path.join(HERE, "ssim_seam.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", os.path.join(HERE, "ssim_seam.json"))


if __name__ == "__main__":
    main()
