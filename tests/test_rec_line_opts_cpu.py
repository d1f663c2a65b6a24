"""The per-line options of the rec tail as one value (retto_amd/csrc/rec_line_opts.h) on the host: how rt_run_regions* resolves
the regions' charset / lexicon / pattern ids (rt::resolve_region_opts), how a call's regions or defaults become one entry per line
(rt::expand_line_opts), and the rule that a line carries at most one of a pattern and a lexicon (rt::rec_opts_conflict).
session.cpp wraps every message below in RT_ERR_INVALID; the GPU pipeline tests match the same texts.  The expected answers are
restated here from the rules, and a handful are written out by hand.  Compiled with g++ into tests/native/gemm_plan_driver.cpp
(tests/plan_driver.py): no GPU."""
import pytest

import plan_driver

KINDS = ("charset", "lexicon", "pattern")
BOTH = "both a rec pattern (%d) and a rec lexicon (%d): a line may not carry both"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


def words(*parts):
    return " ".join(str(w) for part in parts for w in part)


def fmt(opts):
    return ",".join("%d:%d:%d" % tuple(o) for o in opts) if opts else "-"


# ---- regions: (defaults, counts, regions per page, the three arrays: None, or per page None or the regions' ids) ----
def regions_query(dflt, counts, n, arrays):
    w = ["regions"] + list(dflt) + list(counts) + [len(n)] + list(n)
    for a in arrays:
        w.append(0 if a is None else 1)
        for page in a or []:
            w += [0] if page is None else [1] + list(page)
    return words(w)


def regions_expected(dflt, counts, n, arrays):
    """-1 is the default, 0 none, up to the count that id; a missing array or page entry is all -1.  The first error: pages in
    order, inside a page every region's charset, then every lexicon, then every pattern, a region's conflict with its pattern."""
    out = []
    for i in range(len(n)):
        page = [list(dflt) for _ in range(n[i])]
        for j, noun in enumerate(KINDS):
            for k in range(n[i]):
                v = -1 if arrays[j] is None or arrays[j][i] is None else arrays[j][i][k]
                if v < -1 or v > counts[j]:
                    return "error: page %d region %d: unknown %s id %d" % (i, k, noun, v)
                if v >= 0:
                    page[k][j] = v
                if j == 2 and page[k][2] > 0 and page[k][1] > 0:
                    return "error: page %d region %d: " % (i, k) + BOTH % (page[k][2], page[k][1])
        out.append(page)
    return " ".join(["ok"] + [fmt(p) for p in out])


D, C = (1, 2, 0), (3, 2, 4)          # defaults: charset 1, lexicon 2, no pattern; the session holds 3 charsets, 2 lexicons, 4 patterns
N = [3, 0, 1, 2]                     # pages of 3, 0, 1 and 2 regions
REGIONS = [  # (what it pins, defaults, counts, regions per page, charsets, lexicons, patterns)
    ("no array at all: every region the defaults", D, C, N, None, None, None),
    ("arrays of -1 are no array", D, C, N, [[-1] * 3, [], [-1], [-1, -1]], [[-1] * 3, [], [-1], [-1, -1]], [[-1] * 3, [], [-1], [-1, -1]]),
    ("a null page entry is all -1", D, C, N, [None, None, [3], None], [[0, 1, -1], None, None, [0, 0]], [None] * 4),
    ("0 overrides a non-zero default, per kind", (1, 0, 3), C, [2], [[0, -1]], [[-1, -1]], [[-1, 0]]),
    ("-1 is the default of its own kind", (2, 0, 4), C, [3], [[-1, 3, 0]], [[-1, 0, 2]], [[-1, 1, 0]]),
    ("ids at the count", (0, 0, 0), C, [2], [[3, 0]], [[2, 0]], [[0, 4]]),
    ("a charset at count + 1", (0, 0, 0), C, [1, 3], [None, [3, 4, 0]], None, None),
    ("page 1 region 2: unknown charset id 99", D, C, [1, 3], [[0], [1, 2, 99]], None, None),
    ("page 0 region 5: unknown lexicon id -2", (0, 0, 0), C, [6], None, [[0, 1, 2, -1, 0, -2]], None),
    ("page 0 region 2: unknown pattern id 9", (0, 0, 0), C, [3], None, None, [[1, 4, 9]]),
    ("a lexicon at count + 1", (0, 0, 0), C, [1], None, [[3]], None),
    ("a pattern at count + 1", (0, 0, 0), C, [1], None, None, [[5]]),
    ("-2 in every kind: the charset is reported", (0, 0, 0), C, [1], [[-2]], [[-2]], [[-2]]),
    ("a bad pattern on region 0, a bad charset on region 1: the charset", (0, 0, 0), C, [2], [[0, 7]], None, [[9, 0]]),
    ("a bad lexicon on page 0, a bad charset on page 1: page 0", (0, 0, 0), C, [1, 1], [[0], [7]], [[9], [0]], None),
    ("a region's own pattern and lexicon", (0, 0, 0), C, [2, 3], None, [None, [0, 1, 2]], [None, [3, 0, 4]]),
    ("a default lexicon and a region pattern", (0, 2, 0), C, [3], None, None, [[0, 0, 1]]),
    ("a default pattern and a region lexicon", (0, 0, 3), C, [2], None, [[0, 1]], None),
    ("both defaults, every region overrides one with 0", (0, 1, 1), C, [2], None, [[0, -1]], [[-1, 0]]),
    ("both defaults, a region left alone", (0, 1, 1), C, [2], None, [[0, -1]], [[-1, -1]]),
    ("a conflict on region 0 hides a bad pattern id on region 1", (0, 1, 0), C, [2], None, None, [[2, 9]]),
    ("no page", D, C, [], None, None, None),
]

REGIONS_BY_HAND = {
    "no array at all: every region the defaults": "ok 1:2:0,1:2:0,1:2:0 - 1:2:0 1:2:0,1:2:0",
    "arrays of -1 are no array": "ok 1:2:0,1:2:0,1:2:0 - 1:2:0 1:2:0,1:2:0",
    "a null page entry is all -1": "ok 1:0:0,1:1:0,1:2:0 - 3:2:0 1:0:0,1:0:0",
    "0 overrides a non-zero default, per kind": "ok 0:0:3,1:0:0",
    "ids at the count": "ok 3:2:0,0:0:4",
    "a charset at count + 1": "error: page 1 region 1: unknown charset id 4",
    "page 1 region 2: unknown charset id 99": "error: page 1 region 2: unknown charset id 99",
    "page 0 region 5: unknown lexicon id -2": "error: page 0 region 5: unknown lexicon id -2",
    "page 0 region 2: unknown pattern id 9": "error: page 0 region 2: unknown pattern id 9",
    "-2 in every kind: the charset is reported": "error: page 0 region 0: unknown charset id -2",
    "a bad pattern on region 0, a bad charset on region 1: the charset": "error: page 0 region 1: unknown charset id 7",
    "a bad lexicon on page 0, a bad charset on page 1: page 0": "error: page 0 region 0: unknown lexicon id 9",
    "a region's own pattern and lexicon": "error: page 1 region 2: both a rec pattern (4) and a rec lexicon (2): a line may not carry both",
    "a default lexicon and a region pattern": "error: page 0 region 2: both a rec pattern (1) and a rec lexicon (2): a line may not carry both",
    "both defaults, every region overrides one with 0": "ok 0:0:1,0:1:0",
    "a conflict on region 0 hides a bad pattern id on region 1": "error: page 0 region 0: both a rec pattern (2) and a rec lexicon (1): a line may not carry both",
    "no page": "ok",
}


@pytest.fixture(scope="module")
def region_answers(exe):
    return plan_driver.run(exe, [regions_query(d, c, n, (cs, lx, pt)) for _, d, c, n, cs, lx, pt in REGIONS])


@pytest.mark.parametrize("i", range(len(REGIONS)), ids=[c[0] for c in REGIONS])
def test_regions_resolve_by_the_rules(region_answers, i):
    _, d, c, n, cs, lx, pt = REGIONS[i]
    assert region_answers[i] == regions_expected(d, c, n, (cs, lx, pt))


@pytest.mark.parametrize("what", sorted(REGIONS_BY_HAND))
def test_regions_by_hand(region_answers, what):
    assert region_answers[[c[0] for c in REGIONS].index(what)] == REGIONS_BY_HAND[what]


# ---- lines: (defaults, counts, boxes per page, None = the defaults, or per page every box's (charset, lexicon, pattern)) ----
def lines_query(dflt, counts, n, page_opts):
    w = ["lines"] + list(dflt) + list(counts) + [len(n)] + list(n) + [0 if page_opts is None else 1]
    for page in page_opts or []:
        for o in page:
            w += list(o)
    return words(w)


def lines_expected(dflt, counts, n, page_opts):
    """Line k of page i is line (boxes of the earlier pages) + k; without regions every line is the defaults.  The first id outside
    [0, count]: every line's charset, then every lexicon, then every pattern; then the first line with a pattern and a lexicon."""
    lines = [tuple(o) for page in page_opts for o in page] if page_opts is not None else [tuple(dflt)] * sum(n)
    for j, noun in enumerate(KINDS):
        for o in lines:
            if o[j] < 0 or o[j] > counts[j]:
                return "error: unknown rec %s id %d" % (noun, o[j])
    for li, o in enumerate(lines):
        if o[2] > 0 and o[1] > 0:
            return "error: line %d carries both a rec pattern and a rec lexicon" % li
    return "any=%d,%d,%d lines=%s" % tuple([int(any(o[j] > 0 for o in lines)) for j in range(3)] + [fmt(lines)])


B = [0, 1, 3]                        # pages of 0, 1 and 3 boxes
LINES = [  # (what it pins, defaults, counts, boxes per page, the pages' resolved options or None)
    ("the defaults on every line", D, C, B, None),
    ("no default at all: every any is 0", (0, 0, 0), C, B, None),
    ("regions, every id 0: every any is 0, whatever the defaults", D, C, B, [[], [(0, 0, 0)], [(0, 0, 0)] * 3]),
    ("regions: a line's options are its region's", D, C, B, [[], [(3, 0, 0)], [(0, 2, 0), (0, 0, 0), (1, 0, 4)]]),
    ("regions: a lexicon on the last line only", (0, 0, 0), C, B, [[], [(0, 0, 0)], [(0, 0, 0), (0, 0, 0), (0, 1, 0)]]),
    ("regions: a pattern on the first line only", (0, 0, 0), C, [1, 0, 3], [[(0, 0, 2)], [], [(0, 0, 0)] * 3]),
    ("a default pattern alone", (0, 0, 4), C, [2], None),
    ("NL == 0 with defaults: nothing has anything", D, C, [0, 0], None),
    ("NL == 0 with regions", D, C, [0], [[]]),
    ("no page", D, C, [], None),
    ("NL == 0: defaults that conflict do not matter to the lines", (0, 1, 1), C, [0], None),
    ("a default beyond the count", (4, 0, 0), C, [1], None),
    ("a lexicon beyond the count is reported behind every charset", (0, 0, 0), C, [2], [[(0, 3, 0), (0, 0, 0)]]),
    ("a bad pattern on line 0, a bad charset on line 1: the charset", (0, 0, 0), C, [2], [[(0, 0, 5), (-1, 0, 0)]]),
    ("the second line carries both", (0, 0, 0), C, [1, 1], [[(1, 2, 0)], [(0, 2, 4)]]),
    ("defaults that carry both", (0, 2, 4), C, B, None),
]
LINES_BY_HAND = {
    "the defaults on every line": "any=1,1,0 lines=1:2:0,1:2:0,1:2:0,1:2:0",
    "no default at all: every any is 0": "any=0,0,0 lines=0:0:0,0:0:0,0:0:0,0:0:0",
    "regions, every id 0: every any is 0, whatever the defaults": "any=0,0,0 lines=0:0:0,0:0:0,0:0:0,0:0:0",
    "regions: a line's options are its region's": "any=1,1,1 lines=3:0:0,0:2:0,0:0:0,1:0:4",
    "regions: a lexicon on the last line only": "any=0,1,0 lines=0:0:0,0:0:0,0:0:0,0:1:0",
    "NL == 0 with defaults: nothing has anything": "any=0,0,0 lines=-",
    "NL == 0 with regions": "any=0,0,0 lines=-",
    "a default beyond the count": "error: unknown rec charset id 4",
    "a bad pattern on line 0, a bad charset on line 1: the charset": "error: unknown rec charset id -1",
    "the second line carries both": "error: line 1 carries both a rec pattern and a rec lexicon",
    "defaults that carry both": "error: line 0 carries both a rec pattern and a rec lexicon",
}


@pytest.fixture(scope="module")
def line_answers(exe):
    return plan_driver.run(exe, [lines_query(d, c, n, po) for _, d, c, n, po in LINES])


@pytest.mark.parametrize("i", range(len(LINES)), ids=[c[0] for c in LINES])
def test_lines_expand_by_the_rules(line_answers, i):
    assert line_answers[i] == lines_expected(*LINES[i][1:])


@pytest.mark.parametrize("what", sorted(LINES_BY_HAND))
def test_lines_by_hand(line_answers, what):
    assert line_answers[[c[0] for c in LINES].index(what)] == LINES_BY_HAND[what]


def test_session_defaults_may_not_carry_both(exe):
    """The form of the rule for the session defaults (rt_run_batch, rt_submit_batch): a pattern and a lexicon, never a charset."""
    got = plan_driver.run(exe, ["defaults 0 0 0", "defaults 3 2 0", "defaults 3 0 4", "defaults 0 2 4", "defaults 1 1 1"])
    assert got[:3] == ["ok"] * 3
    assert got[3] == "error: the session defaults name both a rec pattern (4) and a rec lexicon (2): a line may not carry both"
    assert got[4] == "error: the session defaults name both a rec pattern (1) and a rec lexicon (1): a line may not carry both"
