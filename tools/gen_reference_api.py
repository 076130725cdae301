"""Record the reference package's public API as names only (``tests/golden/reference_api.json``), so that
``tests/unittests/misc/test_module_paths.py`` needs no reference tree:

* ``modules``: for every module file (relative path), the public classes / functions defined at its top level;
* ``signatures``: for every public function, or class with an ``__init__`` / ``__new__``, its argument names.

Usage: python tools/gen_reference_api.py <reference>/src/torchmetrics [out.json]
"""
import ast
import json
import os
import sys


def _parse(path: str) -> ast.Module:
    with open(path) as fh:
        return ast.parse(fh.read())


def modules(ref: str) -> dict:
    out = {}
    for dp, _, fn in os.walk(ref):
        for f in sorted(fn):
            if f.endswith(".py") and f != "__init__.py" and f != "__about__.py":
                tree = _parse(os.path.join(dp, f))
                rel = os.path.relpath(os.path.join(dp, f), ref)
                out[rel] = [n.name for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and not n.name.startswith("_")]
    return dict(sorted(out.items()))


def signatures(ref: str) -> dict:
    defs = {}
    for dp, dn, fn in os.walk(ref):
        dn.sort()
        for f in sorted(fn):
            if not f.endswith(".py") or f.startswith("_deprecated"):
                continue
            for n in _parse(os.path.join(dp, f)).body:
                if isinstance(n, ast.FunctionDef) and not n.name.startswith("_"):
                    defs.setdefault(n.name, n)
                if isinstance(n, ast.ClassDef) and not n.name.startswith("_"):
                    ctor = [b for b in n.body if isinstance(b, ast.FunctionDef) and b.name in ("__init__", "__new__")]
                    if ctor:
                        defs[n.name] = ctor[-1]
    return {k: [a.arg for a in v.args.args + v.args.kwonlyargs if a.arg not in ("self", "cls")] for k, v in sorted(defs.items())}


def main() -> None:
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_api.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"modules": modules(ref), "signatures": signatures(ref)}, fh, indent=0, sort_keys=False)
        fh.write("\n")


if __name__ == "__main__":
    main()
