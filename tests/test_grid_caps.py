"""tests/grid_caps.py held against the sources, without a GPU: every cap of the table is the literal in its source line, every capped
launch of the forms the code base uses is a row of the table or a commented exclusion, and every test the table names exists.  A cap
that somebody raises, or a new capped launch, fails here instead of silently turning a second-trip test into a first-trip one."""
import ast
import glob
import os
import re

import pytest

import grid_caps
from conftest import ROOT

CSRC = os.path.join(ROOT, "ideas_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ideas_hip.h")

# The forms a capped launch takes in csrc/*.hip; group n is the cap, a number or a named constant.
FORMS = [
    re.compile(r"if \((?P<x>grid|g|blocks|nblk) > (?P<n>\w+)\) (?P=x) = (?P=n);"),      # if (X > N) X = N;
    re.compile(r"< (?P<n>\d+) \? [^:;]+ : (?P=n)\b"),                                     # a < N ? a : N
    re.compile(r"> (?P<n>\d+) \? (?P=n) : "),                                             # a > N ? N : a
    re.compile(r"\bna_grid\(\w+, (?P<n>\w+)\)"),                                          # na_grid(a, N)
    re.compile(r"constexpr int (?P<n>\w+_MAX_BLOCKS) = "),                                # the *_MAX_BLOCKS constants
]


def sources():
    return {os.path.basename(p): open(p).read().splitlines() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def number(token, lines):
    """The value of a cap: a literal, or a constant of the file, itself a literal or a #define of include/ideas_hip.h."""
    for _ in range(3):
        if token.isdigit():
            return int(token)
        m = [re.search(r"constexpr int %s = (\w+);" % token, ln) for ln in lines]
        m = [x for x in m if x] or [x for x in (re.search(r"#define\s+%s\s+(\w+)" % token, ln) for ln in open(HEADER).read().splitlines()) if x]
        assert len(m) == 1, token
        token = m[0].group(1)
    raise AssertionError(token)


def line_of(row, lines):
    """0-based index of the row's line in its file"""
    at = [i for i, ln in enumerate(lines) if ln.strip() == row.line]
    assert len(at) > row.nth, (row.file, row.line, "found %d time(s)" % len(at))
    return at[row.nth]


def hits(src=None):
    """(file, 0-based line, cap token) of every line of csrc/*.hip that one of the forms matches"""
    found = []
    for name, lines in (src or sources()).items():
        for i, ln in enumerate(lines):
            code = ln.split("//")[0]
            for form in FORMS:
                m = form.search(code)
                if m:
                    found.append((name, i, m.group("n")))
                    break
    return found


def test_the_table_has_rows_and_every_row_is_sane():
    assert len(grid_caps.CAPS) >= 40
    for key, row in grid_caps.CAPS.items():
        assert row.cap > 0 and row.units > 0 and row.unit and row.site, key
        assert re.fullmatch(r"tests/test_\w+\.py::test_\w+", row.test), key


@pytest.mark.parametrize("key", sorted(grid_caps.CAPS))
def test_the_cap_is_the_literal_in_the_source(key):
    row = grid_caps.CAPS[key]
    lines = sources()[row.file]
    ln = lines[line_of(row, lines)]
    m = [f.search(ln.split("//")[0]) for f in FORMS]
    m = [x for x in m if x]
    assert m, (key, "the line has none of the forms", ln)
    assert number(m[0].group("n"), lines) == row.cap, (key, ln, row.cap)
    assert any(row.site in other for other in lines), (key, row.site, "is not in", row.file)


def test_every_capped_launch_is_a_row_or_an_exclusion():
    src = sources()
    claimed = {(row.file, line_of(row, src[row.file])) for row in grid_caps.CAPS.values()}
    named = {(row.file, tok) for row in grid_caps.CAPS.values() for tok in re.findall(r"\w+_MAX_BLOCKS", row.line)}
    used = set()
    for name, i, token in hits(src):
        text = src[name][i].strip()
        if (name, i) in claimed:
            continue
        if FORMS[4].search(text) and (name, token) in named:         # a constant that a row's line names
            continue
        excl = [k for k in grid_caps.EXCLUDED if k[0] == name and k[1] in text]
        assert excl, "%s:%d is a capped launch without a row in tests/grid_caps.py: %s" % (name, i + 1, text)
        used.update(excl)
    assert used == set(grid_caps.EXCLUDED), ("exclusions that match nothing", set(grid_caps.EXCLUDED) - used)
    for why in grid_caps.EXCLUDED.values():
        assert len(why) > 10


def test_the_search_finds_what_it_is_for():
    """One line of each form, and the limits that are no caps."""
    probe = {"x.hip": ["    if (grid > 16384) grid = 16384;", "    if (nblk > LP_MAX_BLOCKS) nblk = LP_MAX_BLOCKS;",
                       "static unsigned tile_grid(int64_t ntiles) { return (unsigned)(ntiles < 65536 ? ntiles : 65536); }",
                       "    d->nblocks = (int)(items / 256 + 1 < 2048 ? items / 256 + 1 : 2048);", "    return (unsigned)(grid > 16384 ? 16384 : grid);",
                       "    const dim3 grid(na_grid(a, 4096));", "constexpr int NA_MAX_BLOCKS = IDEAS_NOISE_ACT_MAX_PARTIALS;",
                       "    const int qscale = quality < 50 ? 5000 / quality : 200 - 2 * quality;", "    if (x > 3) y = 3;  // if (grid > 5) grid = 5;"]}
    assert [(i, n) for _, i, n in hits(probe)] == [(0, "16384"), (1, "LP_MAX_BLOCKS"), (2, "65536"), (3, "2048"), (4, "16384"), (5, "4096"),
                                                   (6, "NA_MAX_BLOCKS")]


def test_every_named_test_exists():
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), path)
        defined["tests/" + os.path.basename(path)] = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    for key, row in grid_caps.CAPS.items():
        path, name = row.test.split("::")
        assert name in defined.get(path, ()), (key, row.test)
