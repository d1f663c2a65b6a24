"""The plan of one rec group's CTC tail (retto_amd/csrc/rec_tail_plan.h: rt::rec_tail_plan) on the host: the charset row tables,
the lexicon lines with their rows and table, and the answers that order the launches (a lexicon line at all, a snap group, z5
needed).  rec_groups (session.cpp) and the rt_debug_ctc_* hooks (api_debug.cpp) both run rt_session::rec_tail on this plan, so
what test_gpu_charset.py, test_gpu_lexicon.py and test_gpu_lexicon_align.py certify is what a page runs through.  The expected
tables are restated here (expected()), from the rules of ctc_charset.h / ctc_lexicon.h / ctc_lexicon_align.h, and a few are
written out by hand.  Compiled with g++ into tests/native/gemm_plan_driver.cpp (tests/plan_driver.py): no GPU.

A lexicon of the driver is (n16, n32, n64): its entries of 1, 8 and 16 ids, which fall into the 16-, 32- and 64-lane buckets."""
import pytest

import plan_driver

MAX_GROUP_TABLE = 1 << 26


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return plan_driver.build(tmp_path_factory)


def query(T, l0, l1, sets=None, lexs=None, lexicons=(), snaps=None, cand_k=0):
    def opt(v):
        return ["0"] if v is None else ["1"] + ["%g" % x for x in v]
    words = ["tail", l0, l1, cand_k, len(T)] + list(T) + opt(sets) + opt(lexs) + [len(lexicons)]
    for lex in lexicons:
        words += list(lex)
    return " ".join(str(w) for w in words + opt(snaps))


def expected(T, l0, l1, sets=None, lexs=None, lexicons=(), snaps=None, cand_k=0):
    """The driver's answer, from the rules: rows count from the group's first; a group with a restricted row has every row's set
    and the restricted rows in line order; a lexicon line is (first position in the compact row list, T, lexicon 0-based, line
    index in the call, first float of its loglik row); a wave of the forward kernel carries 4 / 2 / 1 entries of a bucket."""
    first = [sum(T[:i]) - sum(T[:l0]) for i in range(len(T) + 1)]
    group = range(l0, l1)
    crows = [first[i] + t for i in group for t in range(T[i]) if sets and sets[i] > 0]
    row_set = [sets[i] for i in group for _ in range(T[i])] if crows else []
    lines, lrows, table, waves, snap = [], [], 0, 0, False
    for i in group:
        if not lexs or lexs[i] <= 0:
            continue
        n16, n32, n64 = lexicons[lexs[i] - 1]
        lines.append("%d:%d:%d:%d:%d" % (len(lrows), T[i], lexs[i] - 1, i, table))
        lrows += [first[i] + t for t in range(T[i])]
        table += n16 + n32 + n64
        waves = max(waves, (n16 + 3) // 4 + (n32 + 1) // 2 + n64)
        snap = snap or bool(snaps and snaps[lexs[i] - 1] > 0)

    def lst(v):
        return ",".join(str(x) for x in v) if v else "-"
    return "rows=%d z5=%d has_lex=%d snap=%d table=%d fits=%d max_waves=%d row_set=%s crows=%s lines=%s lrows=%s" % (
        first[l1], int(cand_k > 1 or bool(crows) or bool(lines)), int(bool(lines)), int(snap), table, int(table <= MAX_GROUP_TABLE), waves,
        lst(row_set), lst(crows), lst(lines), lst(lrows))


T5 = [2, 1, 3, 65, 4]                 # lines of 1, 3 and 64 + 1 time steps inside the group [1, 4); lines 0 and 4 outside it
A, B = (9, 0, 0), (1, 1, 2)           # two bucket mixes: A has more entries and 3 waves, B has 4 entries and 1 + 1 + 2 = 4 waves
FULL = (65536, 0, 0)                  # RT_LEXICON_MAX_ENTRIES entries: 1024 lines of it fill a group's table exactly

CASES = [  # (what it pins, keyword arguments of query() / expected())
    ("nothing on", dict(T=T5, l0=1, l1=4)),
    ("nothing on, K = 1: ranks 0 need no logits", dict(T=T5, l0=1, l1=4, cand_k=1)),
    ("nothing on, K = 2: z5 for the candidates alone", dict(T=T5, l0=1, l1=4, cand_k=2)),
    ("arrays given, every id 0", dict(T=T5, l0=1, l1=4, sets=[0] * 5, lexs=[0] * 5, lexicons=[A])),
    ("a set on the first line of the group", dict(T=T5, l0=1, l1=4, sets=[0, 2, 0, 0, 0])),
    ("a set on the last line of the group", dict(T=T5, l0=1, l1=4, sets=[0, 0, 0, 1, 0])),
    ("sets on lines outside the group only", dict(T=T5, l0=1, l1=4, sets=[3, 0, 0, 0, 3])),
    ("two sets, an unrestricted line between them", dict(T=T5, l0=1, l1=4, sets=[1, 2, 0, 1, 1], cand_k=1)),
    ("the whole call as one group", dict(T=T5, l0=0, l1=5, sets=[1, 0, 2, 0, 3])),
    ("a lexicon line between two plain lines", dict(T=T5, l0=1, l1=4, lexs=[0, 0, 1, 0, 0], lexicons=[A])),
    ("two lexicons: the one with fewer entries decides max_waves", dict(T=T5, l0=1, l1=4, lexs=[0, 1, 0, 2, 0], lexicons=[A, B])),
    ("the same two, the other way round", dict(T=T5, l0=1, l1=4, lexs=[2, 2, 1, 1, 1], lexicons=[A, B])),
    ("lexicon A alone: its own waves", dict(T=T5, l0=1, l1=4, lexs=[2, 1, 1, 1, 2], lexicons=[A, B])),
    ("a lexicon line without a time step still counts", dict(T=[2, 0, 3], l0=0, l1=3, lexs=[0, 1, 0], lexicons=[B])),
    ("sets and lexicons on the same and on different lines", dict(T=T5, l0=1, l1=4, sets=[0, 1, 1, 0, 0], lexs=[0, 0, 2, 1, 0], lexicons=[A, B], cand_k=5)),
    ("snap on a lexicon of a line inside the group", dict(T=T5, l0=1, l1=4, lexs=[1, 0, 2, 1, 0], lexicons=[A, B], snaps=[0, 0.5])),
    ("snap on a lexicon of a line outside the group only", dict(T=T5, l0=1, l1=4, lexs=[2, 0, 1, 1, 2], lexicons=[A, B], snaps=[0, 0.5])),
    ("the same call, the group that holds the snap line", dict(T=T5, l0=4, l1=5, lexs=[2, 0, 1, 1, 2], lexicons=[A, B], snaps=[0, 0.5])),
    ("snap thresholds all 0", dict(T=T5, l0=1, l1=4, lexs=[0, 1, 2, 1, 0], lexicons=[A, B], snaps=[0, 0])),
    ("no snap table at all", dict(T=T5, l0=1, l1=4, lexs=[0, 1, 2, 1, 0], lexicons=[A, B])),
    ("the table exactly at MAX_GROUP_TABLE", dict(T=[1] * 1026, l0=1, l1=1025, lexs=[2] + [1] * 1024 + [2], lexicons=[FULL, (1, 0, 0)])),
    ("one float more", dict(T=[1] * 1026, l0=1, l1=1026, lexs=[2] + [1] * 1024 + [2], lexicons=[FULL, (1, 0, 0)])),
]


@pytest.fixture(scope="module")
def answers(exe):
    return plan_driver.run(exe, [query(**kw) for _, kw in CASES])


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_plan_matches_the_rules(answers, i):
    assert answers[i] == expected(**CASES[i][1])


# the same answers written out, so that a slip shared by expected() and the plan cannot hide
BY_HAND = {
    "nothing on": "rows=69 z5=0 has_lex=0 snap=0 table=0 fits=1 max_waves=0 row_set=- crows=- lines=- lrows=-",
    "nothing on, K = 1: ranks 0 need no logits": "rows=69 z5=0 has_lex=0 snap=0 table=0 fits=1 max_waves=0 row_set=- crows=- lines=- lrows=-",
    "nothing on, K = 2: z5 for the candidates alone": "rows=69 z5=1 has_lex=0 snap=0 table=0 fits=1 max_waves=0 row_set=- crows=- lines=- lrows=-",
    "a set on the first line of the group": "rows=69 z5=1 has_lex=0 snap=0 table=0 fits=1 max_waves=0 row_set=2," + ",".join(["0"] * 68) +
                                            " crows=0 lines=- lrows=-",
    "sets on lines outside the group only": "rows=69 z5=0 has_lex=0 snap=0 table=0 fits=1 max_waves=0 row_set=- crows=- lines=- lrows=-",
    "a lexicon line between two plain lines": "rows=69 z5=1 has_lex=1 snap=0 table=9 fits=1 max_waves=3 row_set=- crows=- lines=0:3:0:2:0 lrows=1,2,3",
    "two lexicons: the one with fewer entries decides max_waves":
        "rows=69 z5=1 has_lex=1 snap=0 table=13 fits=1 max_waves=4 row_set=- crows=- lines=0:1:0:1:0,1:65:1:3:9 lrows=0," +
        ",".join(str(r) for r in range(4, 69)),
    "a lexicon line without a time step still counts": "rows=5 z5=1 has_lex=1 snap=0 table=4 fits=1 max_waves=4 row_set=- crows=- lines=0:0:0:1:0 lrows=-",
    "snap on a lexicon of a line outside the group only":
        "rows=69 z5=1 has_lex=1 snap=0 table=18 fits=1 max_waves=3 row_set=- crows=- lines=0:3:0:2:0,3:65:0:3:9 lrows=" +
        ",".join(str(r) for r in range(1, 69)),
    "the same call, the group that holds the snap line": "rows=4 z5=1 has_lex=1 snap=1 table=4 fits=1 max_waves=4 row_set=- crows=- lines=0:4:1:4:0 lrows=0,1,2,3",
}


@pytest.mark.parametrize("what", sorted(BY_HAND))
def test_plan_by_hand(answers, what):
    assert answers[[c[0] for c in CASES].index(what)] == BY_HAND[what]


def test_table_capacity_edge(answers):
    """1024 lines of a 65536-entry lexicon are exactly lx::MAX_GROUP_TABLE floats: the group fits; one more line of a one-entry
    lexicon does not, and rec_groups then fails with RT_ERR_CAPACITY."""
    at, over = (answers[[c[0] for c in CASES].index(w)] for w in ("the table exactly at MAX_GROUP_TABLE", "one float more"))
    assert "table=%d fits=1 " % MAX_GROUP_TABLE in at and "rows=1024 " in at
    assert "table=%d fits=0 " % (MAX_GROUP_TABLE + 1) in over and "rows=1025 " in over
    assert over.split(" lines=")[1].split(" ")[0].endswith(",1024:1:1:1025:%d" % MAX_GROUP_TABLE)
