"""Generate tests/golden/surface_ref.json: the names the reference's text uses on the objects the product provides, collected
with `ast` (nothing of the reference is imported or executed) from a checkout of the reference:

  uses       scripts/check_surface.collect(): every `dsp.<name>`, sub-receiver attribute chain, `psd.<attr>`, ring-buffer
             method, `lo.<attr>` and `convolve_fast` use -> {kind: {name: ["file:line", ...]}}
  sdr_calls  `P.sdr.<method>(...)` / `sdr.<method>(...)` in receiver.py, utils.py:292-460 and soapy.py -> {method: [arities]}

tests/test_surface.py checks the product against this file, so the suite needs no copy of the reference.

    python tests/golden/make_surface_golden.py <reference checkout>
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def sdr_calls(ref):
    calls = {}
    for fn, lo, hi in (("receiver.py", 1, 10 ** 6), ("utils.py", 292, 460), ("soapy.py", 1, 10 ** 6)):
        tree = ast.parse(open(os.path.join(ref, fn)).read())
        for n in ast.walk(tree):
            if not (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and lo <= n.lineno <= hi):
                continue
            v = n.func.value
            if (isinstance(v, ast.Attribute) and v.attr == "sdr") or (isinstance(v, ast.Name) and v.id == "sdr"):
                calls.setdefault(n.func.attr, set()).add(len(n.args))
    return {m: sorted(a) for m, a in sorted(calls.items())}


if __name__ == "__main__":
    ref = sys.argv[1]
    import check_surface
    check_surface.REF = ref
    doc = dict(source="ast walk of the reference's receiver, gui, Plotting, watchdog, utils, pySDR, am, mp, params, srates, "
                      "rtty, hopper, udp, sigs/iq and soapy modules (tests/golden/make_surface_golden.py)",
               uses=check_surface.collect(), sdr_calls=sdr_calls(ref))
    with open(os.path.join(HERE, "surface_ref.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
