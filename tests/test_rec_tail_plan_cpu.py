"""The plan of one rec group's CTC tail (retto_amd/csrc/rec_tail_plan.h: rt::rec_tail_plan) on the host: the charset row tables,
the lexicon lines with their rows and table, and the answers that order the launches (a lexicon line at all, a snap group, z5
needed).  rec_groups (session.cpp) and the rt_debug_ctc_* hooks (api_ctc.cpp) both run rt_session::rec_tail on this plan, so
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


# ---- every kind in one group, and the group's capacity (RecTailPlan::refusal) ----
MAX_GROUP_NODES = 1 << 26
BP_LDS = 8192                         # pt::BP_LDS: a pattern line's backpointer codes up to here stay in the kernel's LDS


def group_query(op, T, l0, l1, opts, lexicons=(), snaps=(), lists=(), pats=(), beam=0, nbest=0):
    """opts: per line (charset, lexicon, pattern, keywords); lexicons / lists: (n16, n32, n64) each; pats: (S, P) each"""
    words = [op, l0, l1, beam, nbest, len(T)] + list(T) + [len(lexicons)]
    for lex in lexicons:
        words += list(lex)
    words += ["%g" % v for v in (snaps or [0] * len(lexicons))] + [len(lists)]
    for kw in lists:
        words += list(kw)
    words += [len(pats)]
    for p in pats:
        words += list(p)
    for o in opts:
        words += list(o)
    return " ".join(str(w) for w in words)


def group_expected(T, l0, l1, opts, lexicons=(), snaps=(), lists=(), pats=(), beam=0, nbest=0):
    """The four line tables of the group from the rules, each kind on its own: a line is (first position in ITS kind's compact row
    list, T, id 0-based or first trie node, line index in the call, its kind's running offset), and its T rows follow the kind's
    earlier lines' rows.  The offsets: a lexicon's / a list's entries; a pattern line's T (P + S) codes where they exceed BP_LDS;
    a beam line's 1 + T B trie nodes (the id) and N T token slots (the offset)."""
    first = [sum(T[:i]) - sum(T[:l0]) for i in range(len(T) + 1)]
    group = range(l0, l1)
    crows = [first[i] + t for i in group for t in range(T[i]) if opts[i][0] > 0]
    row_set = [opts[i][0] for i in group for _ in range(T[i])] if crows else []
    kinds = {k: ([], []) for k in ("lex", "pat", "kw", "beam")}
    table = bp = ktable = nodes = slots = 0

    def add(kind, i, ident, out):
        lines, rows = kinds[kind]
        lines.append("%d:%d:%d:%d:%d" % (len(rows), T[i], ident, i, out))
        rows += [first[i] + t for t in range(T[i])]
    for i in group:
        _, lex, pat, kw = opts[i]
        if lex > 0:
            add("lex", i, lex - 1, table)
            table += sum(lexicons[lex - 1])
        if pat > 0:
            add("pat", i, pat - 1, bp)
            S, P = pats[pat - 1]
            bp += T[i] * (P + S) if T[i] * (P + S) > BP_LDS else 0
        if kw > 0:
            add("kw", i, kw - 1, ktable)
            ktable += sum(lists[kw - 1])
        if beam > 0:
            add("beam", i, nodes, slots)
            nodes += 1 + T[i] * beam
            slots += nbest * T[i]

    def lst(v):
        return ",".join(str(x) for x in v) if v else "-"
    out = " row_set=%s crows=%s" % (lst(row_set), lst(crows))
    for kind, names in (("lex", "lines lrows"), ("pat", "plines prows"), ("kw", "klines krows"), ("beam", "blines brows")):
        out += " %s=%s %s=%s" % (names.split()[0], lst(kinds[kind][0]), names.split()[1], lst(kinds[kind][1]))
    return out


# lines 1 .. 6 of the call are the group: a charset line, a snapping lexicon on a T = 0 line and on a T = 65 line (with keywords),
# a pattern whose 65 (100 + 30) codes leave the LDS and the same pattern short, a keyword line with a charset; the beam on all
COMBINED = dict(T=[2, 3, 0, 65, 65, 4, 1, 5], l0=1, l1=7,
                opts=[(1, 1, 0, 1), (2, 0, 0, 0), (0, 2, 0, 0), (0, 2, 0, 2), (0, 0, 1, 1), (0, 0, 1, 0), (1, 1, 0, 2), (0, 2, 1, 0)],
                lexicons=[A, B], snaps=[0, 0.5], lists=[(3, 0, 0), (2, 1, 0)], pats=[(30, 100)], beam=4, nbest=2)


def test_every_kind_in_one_group(exe):
    """The four kinds share one add(): every table keeps its own row positions and its own offsets."""
    got, = plan_driver.run(exe, [group_query("group", **COMBINED)])
    assert got == group_expected(**COMBINED)
    # ... and by hand: the lexicon lines 2, 3, 6; the pattern lines 4 (8450 codes, past the LDS) and 5; the keyword lines 3, 4, 6;
    # every line with the beam (1 + 4 T nodes, 2 T token slots)
    r = lambda a, b: ",".join(str(v) for v in range(a, b))
    assert got == (" row_set=" + ",".join(["2"] * 3 + ["0"] * 134 + ["1"]) + " crows=0,1,2,137"
                   " lines=0:0:1:2:0,0:65:1:3:4,65:1:0:6:8 lrows=" + r(3, 68) + ",137"
                   " plines=0:65:0:4:0,65:4:0:5:8450 prows=" + r(68, 137) +
                   " klines=0:65:1:3:0,65:65:0:4:3,130:1:1:6:6 krows=" + r(3, 133) + ",137"
                   " blines=0:3:0:1:0,3:0:13:2:6,3:65:14:3:6,68:65:275:4:136,133:4:536:5:266,137:1:553:6:274 brows=" + r(0, 138))


LEX_REFUSAL = ("rec lexicons: 1025 lines of one rec group carry lexicons of 67108865 entries in all, more than the 67108864 likelihoods a "
               "group's table holds: use smaller lexicons or fewer lexicon lines per call")
KW_REFUSAL = ("rec keywords: 1025 lines of one rec group carry keyword lists of 67108865 entries in all, more than the 67108864 scores a "
              "group's table holds: use smaller keyword lists or fewer keyword lines per call")
BEAM_REFUSAL = ("rec beams: the 2048 lines of one rec group need 67108896 trie nodes at beam 32, more than the 67108864 a group's trie "
                "holds: use a narrower beam or fewer lines per call")


def test_capacity_refusals(exe):
    """What rec_groups refuses a group with (RT_ERR_CAPACITY), in full: nothing exactly at each limit, the message one past it,
    and the first in the order lexicons, keywords, beams where several are exceeded.  1024 lines of a 65536-entry list are
    lx::MAX_GROUP_TABLE entries; 2047 lines of 1024 steps and one of 960 are bm::MAX_GROUP_NODES nodes at beam 32 (1 + 32 T each)."""
    two = [FULL, (1, 0, 0)]
    ones = lambda n, **kw: dict(T=[1] * n, l0=0, l1=n, **kw)
    lex = lambda n: ones(n, opts=[(0, 1, 0, 0)] * 1024 + [(0, 2, 0, 0)] * (n - 1024), lexicons=two)
    kws = lambda n: ones(n, opts=[(0, 0, 0, 1)] * 1024 + [(0, 0, 0, 2)] * (n - 1024), lists=two)
    beams = lambda last, opts=None, **kw: dict(T=[1024] * 2047 + [last], l0=0, l1=2048, opts=opts or [(0, 0, 0, 0)] * 2048, beam=32, nbest=1, **kw)
    assert 2047 * (1 + 32 * 1024) + 1 + 32 * 960 == MAX_GROUP_NODES
    both = ones(1025, opts=[(0, 1, 0, 1)] * 1024 + [(0, 2, 0, 2)], lexicons=two, lists=two)
    kw_and_beam = beams(961, opts=[(0, 0, 0, 1)] * 1024 + [(0, 0, 0, 2)] + [(0, 0, 0, 0)] * 1023, lists=two)
    all_three = beams(961, opts=[(0, 1, 0, 1)] * 1024 + [(0, 2, 0, 2)] + [(0, 0, 0, 0)] * 1023, lexicons=two, lists=two)
    cases = [lex(1024), lex(1025), kws(1024), kws(1025), beams(960), beams(961), both, kw_and_beam, all_three]
    got = plan_driver.run(exe, [group_query("capacity", **c) for c in cases])
    assert got == ["-", LEX_REFUSAL, "-", KW_REFUSAL, "-", BEAM_REFUSAL, LEX_REFUSAL, KW_REFUSAL, LEX_REFUSAL]
