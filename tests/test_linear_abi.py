"""CPU: the eight linear entry points are declared, bound and exported, and the build's resource report lists every
k_lincomb instantiation without scratch or spills (a run-time-indexed operand array would show there).  On the parent of
the commit that introduced this file both tests fail: no such names, no such kernels."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lumen_add", "lumen_sub", "lumen_mul_scalar", "lumen_mul_scalar_then_add", "lumen_linear_combination",
         "lumen_add_plain", "lumen_sub_plain", "lumen_mul_plain_then_add")


def test_names_declared_bound_and_exported():
    from lumenos_amd import hip
    lib = hip.load()
    hdr = open(os.path.join(ROOT, "include", "lumenos_hip.h")).read()
    for n in NAMES:
        assert n in hip.SYMBOLS and hasattr(lib, n) and re.search(r"\bint " + n + r"\(", hdr), n
    assert "#define LUMEN_ABI_VERSION 4" in hdr  # new symbols only
    for method in ("add", "sub", "mul_scalar", "mul_scalar_then_add", "linear_combination", "add_plain", "sub_plain",
                   "mul_plain_then_add"):
        assert callable(getattr(hip.Context, method)), method


def test_lincomb_kernels_use_no_scratch():
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    lincomb = {k: v for k, v in rep.items() if "k_lincomb" in k}
    assert len(lincomb) == 8, sorted(lincomb)  # NT = 1 .. 8
    plain = {k: v for k, v in rep.items() if "k_plain_linear" in k}
    assert len(plain) == 2, sorted(plain)
    for k, v in {**lincomb, **plain}.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
