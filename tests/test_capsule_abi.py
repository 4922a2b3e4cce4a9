"""C-ABI 104: the capsule entry points exist in the header, the binding and the library."""
import os
import re

from common import ROOT


def test_capsule_symbols_and_version():
    from flobaroid_amd import _lib

    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "fbr.h")).read()
    for name in ("fbr_model_set_capsules", "fbr_candidate_capsule_distances"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES and re.search(r"\bint " + name + r"\(", hdr), name
    assert lib.fbr_version() == _lib.FBR_VERSION == 104 == int(re.search(r"#define FBR_VERSION (\d+)", hdr).group(1))
    caps, pairs = (int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) for k in ("FBR_MAX_CAPSULES", "FBR_MAX_CAPSULE_PAIRS"))
    assert caps >= 4 * 48 and pairs >= 16 * 1128  # a capsule per link and every link pair of the 48-link WALK-MAN, with room to spare
    assert hasattr(_lib.Engine, "set_capsules") and hasattr(_lib.Engine, "candidate_capsule_distances")
