"""How a batch's pages go over the session's lanes (retto_amd/csrc/lane_split.h) on the host: rt::lanes_for, the number of lanes a
call uses, and rt::lane_split, the contiguous range of pages each lane gets.  The expected answers are restated here from the
rule with the same double operations in the same order (Python floats are doubles), and a table is written out by hand.
Compiled with g++ into tests/native/gemm_plan_driver.cpp (tests/plan_driver.py): no GPU."""
import random

import pytest

import plan_driver

DEFAULT_ACTIVE = 1 << 30   # rt_session::active_lanes before any rt_set_lanes


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


def query(lanes, active, max_side_len, nl, pages):
    return " ".join(str(v) for v in ["split", lanes, active, max_side_len, nl, len(pages)] + [x for hw in pages for x in hw])


def ask(exe, queries):
    """-> per query (lanes_for, first)"""
    out = [[int(v) for v in line.split()] for line in plan_driver.run(exe, queries)]
    return [(a[0], a[1:]) for a in out]


def lanes_for_expected(lanes, active, n_pages):
    return max(1, min(lanes, active, max(n_pages, 1)))


def lane_split_expected(pages, max_side_len, nl):
    """A page's cost: its pixels after the session size limit plus a constant for its lines.  Range l - 1 closes after page i once
    the running cost reaches l / nl of the total, or when every later lane needs one of the pages left."""
    n = len(pages)
    cost, total = [], 0.0
    for h, w in pages:
        h, w = float(max(h, 1)), float(max(w, 1))
        r = min(1.0, float(max_side_len) / max(h, w))
        cost.append(h * w * r * r + 250000.0)
        total += cost[-1]
    first = [0] * (nl + 1)
    acc, l = 0.0, 1
    for i in range(n):
        if l >= nl:
            break
        acc += cost[i]
        if acc >= total * l / nl - 1e-6 or n - (i + 1) <= nl - l:
            first[l] = i + 1
            l += 1
    for k in range(l, nl + 1):
        first[k] = n
    for k in range(1, nl + 1):
        first[k] = max(first[k], first[k - 1])
    return first


TABLE = [  # (pages as (h, w), lanes, max_side_len, first)
    ([(960, 960)] * 32, 3, 2000, [0, 11, 22, 32]),
    ([(480, 640)] * 3, 3, 2000, [0, 1, 2, 3]),
    ([(480, 640)] * 7, 3, 2000, [0, 3, 5, 7]),
    ([(480, 640)] * 5, 2, 2000, [0, 3, 5]),
    ([(100, 100)], 1, 2000, [0, 1]),
    ([(2000, 2000)] + [(500, 500)] * 3, 3, 4000, [0, 1, 2, 4]),
    ([(500, 500)] * 3 + [(2000, 2000)], 3, 4000, [0, 2, 3, 4]),
    ([(4000, 4000)] + [(500, 500)] * 3, 3, 2000, [0, 1, 2, 4]),   # the size limit at work: the large page counts as 2000 x 2000
]


@pytest.mark.parametrize("pages,nl,max_side_len,first", TABLE, ids=[str(i) for i in range(len(TABLE))])
def test_lane_split_table(exe, pages, nl, max_side_len, first):
    assert lane_split_expected(pages, max_side_len, nl) == first
    [(_, got)] = ask(exe, [query(nl, DEFAULT_ACTIVE, max_side_len, nl, pages)])
    assert got == first


def test_lane_split_random_pages_leave_no_lane_empty(exe):
    rng = random.Random(20261020)
    cases = []
    for _ in range(300):
        nl = rng.randint(1, 4)
        n = rng.randint(nl, nl + 12)
        side = lambda: rng.choice([1, 30, 100, 480, 736, 960, 2000, 2001, 4096, rng.randint(1, 5000)])
        cases.append((nl, rng.choice([736, 2000, 4000]), [(side(), side()) for _ in range(n)]))
    answers = ask(exe, [query(nl, DEFAULT_ACTIVE, msl, nl, pages) for nl, msl, pages in cases])
    for (nl, msl, pages), (_, first) in zip(cases, answers):
        assert len(first) == nl + 1 and first[0] == 0 and first[nl] == len(pages), (nl, msl, pages, first)
        assert all(a < b for a, b in zip(first, first[1:])), (nl, msl, pages, first)
        assert first == lane_split_expected(pages, msl, nl), (nl, msl, pages)


def test_lanes_for(exe):
    cases = [(lanes, active, n) for lanes in (1, 2, 3, 4) for active in (1, 2, 3, 5, DEFAULT_ACTIVE) for n in (0, 1, 2, 3, 4, 32)]
    answers = ask(exe, [query(lanes, active, 2000, 1, [(480, 640)] * n) for lanes, active, n in cases])
    for (lanes, active, n), (got, _) in zip(cases, answers):
        assert got == lanes_for_expected(lanes, active, n), (lanes, active, n)
    # by hand: no page still takes a lane; rt_set_lanes below the session's lanes caps them; the default never does
    by_hand = {(3, DEFAULT_ACTIVE, 0): 1, (3, 2, 32): 2, (3, DEFAULT_ACTIVE, 32): 3, (4, DEFAULT_ACTIVE, 2): 2, (4, 1, 4): 1}
    for key, want in by_hand.items():
        assert answers[cases.index(key)][0] == want, key
