"""The bf16x6 product order and its primitives are written once: the sources under
csrc/ call the 32x32x16 bf16 MFMA only from bf16x6.h (and agg_pairwise.hip, whose
four-product hi/lo scheme is its own), and make_rsrc and each form of the split
have one definition."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "multimodal-fl-security_amd", "csrc")
MFMA = "__builtin_amdgcn_mfma_f32_32x32x16_bf16"


def _sources():
    paths = sorted(p for ext in ("h", "hip", "cpp", "hpp", "inc")
                   for p in glob.glob(os.path.join(CSRC, "**", "*." + ext), recursive=True))
    assert len(paths) > 40  # the directory was found
    return {os.path.relpath(p, CSRC): open(p).read() for p in paths}


def _definitions(name):
    """Files that define a function `name`: the name, a parameter list and a body, with something
    that is not a statement (a return type, whatever its qualifiers) before the name on its line —
    a call is preceded by `=`, `(`, `,`, `;`, `return` or nothing."""
    pat = re.compile(r"^[ \t]*(?!return\b)[A-Za-z_][\w:<>,&*\s\[\]()]*?[\w>&*\]]\s+[&*]?" + name +
                     r"\s*\([^;{}]*\)\s*(?:const\s*)?(?:noexcept\s*)?\{", re.M)
    return sorted((f, len(pat.findall(s))) for f, s in _sources().items() if pat.search(s))


def test_the_mfma_is_issued_from_one_header():
    users = sorted(f for f, s in _sources().items() if MFMA in s)
    assert users == ["agg_pairwise.hip", "bf16x6.h"]


def test_the_product_order_is_one_table():
    text = _sources()["bf16x6.h"]
    tables = re.findall(r"X6_ORDER\[6\]\[2\]\s*=\s*\{([^;]*)\};", text)
    assert len(tables) == 1
    pairs = [tuple(int(x) for x in p) for p in re.findall(r"\{\s*(\d)\s*,\s*(\d)\s*\}", tables[0])]
    # term 0 = hi, 1 = mid, 2 = lo; small terms first: mid*mid, hi*lo, lo*hi, hi*mid, mid*hi, hi*hi
    assert pairs == [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)]


def test_primitives_are_defined_once():
    for name in ("make_rsrc", "split3_dot2", "split3_sub", "split1_sub"):
        assert _definitions(name) == [("bf16x6.h", 1)], name
    # no private copy under the old names
    for name in ("split3", "split1"):
        assert _definitions(name) == [], name
