"""The Python surface of gpupathtracer_amd.lib, pinned: tests/data/binding_surface.json lists every public name of the façade and
the signature of every public function and of every public method of Tracer, MultiTracer and SceneFile, as recorded before lib.py
was cut into _abi / host / tracer.  The façade must keep offering at least those names, with equal signatures.

`python tests/test_binding_surface.py` rewrites the fixture from the tree it runs in."""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "data", "binding_surface.json")
CLASSES = ("Tracer", "MultiTracer", "SceneFile")


def surface(lib):
    # (of the modules lib imports, C, T and np are part of the surface: tests and tools spell lib.C.byref, lib.T.X, lib.np.X)
    names = sorted(n for n, v in vars(lib).items() if not n.startswith("_") and (not inspect.ismodule(v) or n in ("C", "T", "np")))
    functions = {n: str(inspect.signature(getattr(lib, n))) for n in names if inspect.isfunction(getattr(lib, n))}
    methods = {c: {n: str(inspect.signature(f)) for n, f in sorted(vars(getattr(lib, c)).items())
                   if inspect.isfunction(f) and not n.startswith("_")} for c in CLASSES}
    return {"names": names, "functions": functions, "methods": methods}


def test_facade_keeps_every_recorded_name_and_signature():
    from gpupathtracer_amd import lib
    recorded = json.load(open(FIXTURE))
    now = surface(lib)
    assert {"C", "T", "np", "LIB_PATH", "EXPORTS", "load", "Tracer", "MultiTracer", "SceneFile"} <= set(recorded["names"])
    assert set(recorded["names"]) <= set(now["names"]), sorted(set(recorded["names"]) - set(now["names"]))
    for name, sig in recorded["functions"].items():
        assert now["functions"].get(name) == sig, name
    for cls in CLASSES:
        for name, sig in recorded["methods"][cls].items():
            assert now["methods"][cls].get(name) == sig, f"{cls}.{name}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from gpupathtracer_amd import lib
    with open(FIXTURE, "w") as f:
        json.dump(surface(lib), f, indent=1, sort_keys=True)
        f.write("\n")
