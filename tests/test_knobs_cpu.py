"""The environment variables the package reads are the ones INTEGRATION.md §5 documents, and the retired A/B knobs stay retired
(source text only, no GPU)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "macarons_amd")

# rows of the §5 table about variables that only bench.py or the tests' helper processes read
BENCH_OR_TEST_ONLY = {"MCR_BENCH_SPIN_SYNC", "MCR_TEST_BACKEND"}

# settled in favour of the default (NOTES.md, "Retired A/B knobs"): each kept a second launch sequence alive that nothing ran
RETIRED = """MCR_SMALL_SPLIT MCR_HEAD_SPLIT MCR_ATTN_PVH MCR_ENC_PLANES MCR_ENDS_PLANES MCR_ENC_ATT_PLANES MCR_ENC_ATT_SPLIT
MCR_ENC_COMBINE_PLANES MCR_HEAD_FUSE_TAIL MCR_HEAD_PLANES MCR_OCC_X_SIDE MCR_OCC_X_EARLY MCR_OCC_BATCH_LOCAL
MCR_KNN_MFMA MCR_KNN_SEG_SPLIT MCR_KNN_SEG_CAND MCR_KNN_GRID MCR_KNN_PARK
MCR_SMALLK_ROWS MCR_LINEAR3 MCR_ATTN_MFMA MCR_ATTN_QG2
MCR_L3_SHORTK MCR_L3_XCD MCR_L3_XCD_MIN MCR_L3P_SMALL MCR_L3P_ONCE
MCR_NBV_SIDE MCR_OCC_BEGIN""".split()

NAME = r"MCR_[A-Z0-9_]+"


def _text(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources(*patterns):
    return sorted(p for pat in patterns for p in glob.glob(os.path.join(PKG, pat), recursive=True))


def names_read():
    """every MCR_* name behind a getenv( in the C++ / HIP sources or on a line that reads os.environ in the Python ones"""
    names = set()
    for p in _sources("csrc*/**/*.hip", "csrc*/**/*.h", "csrc*/**/*.cpp", "csrc*/**/*.inc"):
        names.update(re.findall(r'getenv\(\s*"(%s)"' % NAME, _text(p)))
    for p in _sources("**/*.py"):
        for line in _text(p).splitlines():
            if "os.environ" in line:
                names.update(re.findall(r'["\'](%s)["\']' % NAME, line))
    return names


def names_documented():
    """the MCR_* names in the first cell of the `env` rows of INTEGRATION.md §5"""
    section = re.search(r"^## 5\. Knobs$(.*?)(?=^## |\Z)", _text(os.path.join(ROOT, "INTEGRATION.md")), re.S | re.M).group(1)
    names = set()
    for line in section.splitlines():
        if line.startswith("| env "):
            names.update(re.findall(NAME, line.split("|")[1]))
    return names


def test_the_variables_read_are_the_variables_documented():
    read, documented = names_read(), names_documented()
    assert len(read) >= 10 and BENCH_OR_TEST_ONLY <= documented      # (both scans found their material)
    assert read == documented - BENCH_OR_TEST_ONLY, (f"read but not in INTEGRATION.md §5: {sorted(read - documented)}; "
                                                     f"documented but not read: {sorted(documented - BENCH_OR_TEST_ONLY - read)}")


def test_no_retired_knob_is_named_in_the_package():
    assert len(RETIRED) == 29
    found = []
    for p in _sources("**/*.py", "**/*.hip", "**/*.h", "**/*.cpp", "**/*.inc"):
        txt = _text(p)
        found += [(os.path.relpath(p, ROOT), n) for n in RETIRED if re.search(n + r"(?![A-Z0-9_])", txt)]
    assert not found, found
