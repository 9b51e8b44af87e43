"""CPU: the two entry points of the dot product with one relinearisation per sum are declared, bound and exported,
Context has their methods, and the build's resource report lists every k_tensor_dot and k_dot_fold instantiation without scratch or
spills (the loop over the terms keeps two terms' loads and three wide sums per word in registers).  On the parent of the
commit that introduced this file both tests fail: no such names, no such kernels."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lumen_mul_relin_dot", "lumen_mul_tensor_dot")


def test_names_declared_bound_and_exported():
    from lumenos_amd import hip
    lib = hip.load()
    hdr = open(os.path.join(ROOT, "include", "lumenos_hip.h")).read()
    for n in NAMES:
        assert n in hip.SYMBOLS and hasattr(lib, n) and re.search(r"\bint " + n + r"\(", hdr), n
    assert "#define LUMEN_ABI_VERSION 4" in hdr  # new symbols only
    for method in ("mul_relin_dot", "mul_tensor_dot"):
        assert callable(getattr(hip.Context, method)), method


def test_tensor_dot_kernels_use_no_scratch():
    from lumenos_amd import _build
    _build.build()
    rep = _build.resource_report()
    dot = {k: v for k, v in rep.items() if "k_tensor_dot" in k}
    assert len(dot) == 4, sorted(dot)  # RELIN false / true x 256 / 512 pairs per block
    fold = {k: v for k, v in rep.items() if "k_dot_fold" in k}
    assert len(fold) == 2, sorted(fold)  # RELIN false / true
    for k, v in {**dot, **fold}.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
