#!/usr/bin/env python3
"""Compare the public surface of the Python binding in two trees (no GPU).

    tools/compare_binding.py PARENT_TREE NEW_TREE [--lib libbp_hip.so] > profiles/binding_surface.txt

Each tree is imported in a child process of its own (`import dnnse_amd` from the tree's root).  Of every name of the parent that
does not start with an underscore the report says whether the new tree still has it as the same kind of object with the same
  function / class / public method: inspect.signature and docstring (of a class also which of __enter__ / __exit__ / __del__ it has)
  constant / numpy dtype:           value (a dtype: names, formats, offsets, itemsize)
  ctypes Structure:                 _fields_ with their types, sizeof, docstring
and, after load_library(), of every ABI symbol the restype and argtypes.  --lib: the library both trees load (default: the new
tree's build; the library is the same for both when only the binding changed).  Names and members only the new tree has are listed
as added.  Exit status 1 if a name or member of the parent is missing or differs."""
import argparse
import json
import os
import subprocess
import sys

LIFECYCLE = ("__enter__", "__exit__", "__del__")
TREE = ""          # root of the tree being described: a path under it is the same path in the other tree


def describe(obj):
    import ctypes
    import inspect
    import numpy as np

    def sig(f):
        try:
            return str(inspect.signature(f))
        except (TypeError, ValueError):
            return None
    if inspect.ismodule(obj):
        return {"kind": "module"}
    if inspect.isclass(obj) and issubclass(obj, ctypes.Structure):
        return {"kind": "Structure", "doc": obj.__doc__, "sizeof": ctypes.sizeof(obj), "fields": [[n, t.__name__] for n, t in obj._fields_]}
    if inspect.isclass(obj):
        members = {}
        for n in dir(obj):
            m = inspect.getattr_static(obj, n)
            if not n.startswith("_") or n in LIFECYCLE:
                members[n] = ({"kind": "property", "doc": m.__doc__} if isinstance(m, property) else
                              {"kind": "method", "signature": sig(m), "doc": m.__doc__} if callable(m) else {"kind": "value", "value": repr(m)})
        return {"kind": "class", "doc": obj.__doc__, "signature": sig(obj), "bases": [b.__name__ for b in obj.__mro__ if b.__module__ == "builtins"],
                "members": members}
    if callable(obj):
        return {"kind": "function", "signature": sig(obj), "doc": obj.__doc__}
    if isinstance(obj, np.dtype):
        return {"kind": "dtype", "itemsize": obj.itemsize, "fields": [[n, str(obj.fields[n][0]), obj.fields[n][1]] for n in obj.names]}
    return {"kind": "constant", "value": repr(obj).replace(TREE, "<tree>")}


def dump(tree):
    global TREE
    TREE = tree
    sys.path.insert(0, tree)
    import dnnse_amd as pkg
    out = {"names": {n: describe(getattr(pkg, n)) for n in dir(pkg) if not n.startswith("_")}}
    lib = pkg.load_library()
    name = lambda t: None if t is None else t.__name__
    out["abi"] = {s: {"restype": name(getattr(lib, s).restype), "argtypes": [name(t) for t in getattr(lib, s).argtypes or []]}
                  for s in pkg.ABI_SYMBOLS}
    json.dump(out, sys.stdout)


def compare(where, old, new, lines):
    """Lines for what differs between two descriptions; members and names only `new` has are added, not different."""
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in new:
            lines.append("MISSING  %s" % (where + k))
            bad += 1
        elif k not in old:
            lines.append("added    %s (%s)" % (where + k, new[k].get("kind", "")))
        else:
            a, b = dict(old[k]), dict(new[k])
            ma, mb = a.pop("members", {}), b.pop("members", {})
            if a != b:
                lines.append("DIFFERS  %s\n    parent: %s\n    new:    %s" % (where + k, json.dumps(a, sort_keys=True), json.dumps(b, sort_keys=True)))
                bad += 1
            bad += compare(where + k + ".", ma, mb, lines)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--lib")
    ap.add_argument("--dump", action="store_true", help="print the surface of one tree as JSON (what the child processes run)")
    a = ap.parse_args()
    if a.dump:
        return dump(os.path.abspath(a.parent))
    lib = os.path.abspath(a.lib or os.path.join(a.new, "dnn-for-speech-enhancement_amd", "libbp_hip.so"))
    side = []
    for tree in (a.parent, a.new):
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--dump", tree], env=dict(os.environ, BP_HIP_LIB=lib))
        side.append(json.loads(out))
    lines = []
    bad = compare("", side[0]["names"], side[1]["names"], lines)
    bad += compare("ABI ", side[0]["abi"], side[1]["abi"], lines)
    kinds = {}
    for d in side[0]["names"].values():
        kinds[d["kind"]] = kinds.get(d["kind"], 0) + 1
    print("# public surface of the Python binding: parent commit | this commit (tools/compare_binding.py)")
    print("# parent: %d names (%s), %d ABI symbols; compared: kind, signature, docstring, value, _fields_ / sizeof, restype / argtypes"
          % (len(side[0]["names"]), ", ".join("%d %s" % (v, k) for k, v in sorted(kinds.items())), len(side[0]["abi"])))
    print("\n".join(lines) if lines else "no difference")
    print("# %d of the parent's names, members or symbols missing or different" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
