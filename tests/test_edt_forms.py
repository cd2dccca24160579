"""The batch EDT's form table (edt_forms.py) covers what dispatch can produce, every claim of a case follows from its obstacles
through the host statement of the selection rules, and every case's expected result is right before a GPU sees it: the oracle's
EDT against the closed form with the tie rule, and against the brute force where the volume is small enough."""
import numpy as np
import pytest

import edt_forms as F
from edt_reference import tie_rule_reference
from oracle_py import brute_force_edt

NAMES = [c.name for c in F.CASES]


def test_the_table_holds_the_planned_shapes():
    assert len(set(NAMES)) == len(NAMES)
    assert sorted(set(F.PLAN) - set(NAMES)) == [], "planned shapes the table has lost"
    assert sorted(set(NAMES) - set(F.PLAN)) == [], "cases the plan does not list"


def test_the_table_covers_every_combination_dispatch_can_produce():
    req, imp = F.required_and_impossible()
    assert not (req & set(imp))
    # every form x template combination is either required or listed as impossible with its reason
    allx = {("x", cp, f) for cp in F.CPS for f in ("banded", "windowed", "empty")} | \
           {("x", cp, f, st) for cp in F.CPS for f in ("dnc", "gives_up") for st in ("vec", "dword")}
    allz = {("z", cp, f) for cp in F.CPS for f in ("banded", "windowed", "gives_up", "dnc_direct")}
    allp = {("partial", w, cp, f) for w in ("column", "repair") for cp in F.CPS for f in ("banded", "windowed", "gives_up")}
    for key in allx | allz | allp:
        assert key in req or key in imp, key
    assert all(isinstance(r, str) and r for r in imp.values())
    claimed = set().union(*(c.covers for c in F.CASES))
    assert sorted(claimed & set(imp), key=str) == [], "a case claims a combination that cannot occur"
    assert sorted(claimed - req, key=str) == [], "a case claims a combination nobody asked for"
    assert sorted(req - claimed, key=str) == [], "combinations and patterns no case covers"


def test_the_impossible_combinations_are_impossible_by_the_rules():
    """the reasons, checked where they are arithmetic"""
    assert F.cp_of(F.BAND_MAXK) >= 4                         # more than 160 sites need a line longer than 160: CP >= 4
    for cp, L in ((1, 64), (2, 128)):
        assert F.cp_of(L) == cp and L <= F.BAND_MAXK
    assert not F.update_is_partial((8, 8, 513)) and F.update_is_partial((8, 8, 512))     # CP = 16 of Z is never partial
    assert F.zs_mode(8, 63) == 0 and 63 <= F.BAND_MAXK      # no streaming form below Z = 64, which has no 161 planes
    # a plane without an obstacle gives no row to pass X, and a plane with one gives every row a site
    occ = np.zeros((2, 5, 70), bool)
    occ[0, 4, 69] = True
    form, _ = F.row_forms_x(occ)
    assert set(form[0]) == {"banded"} and set(form[1]) == {"skipped"}


# (size, full, completion, guess, kernels); test_edt_plan_host.py holds the product's plan against every row too
HAND_ROWS = [
    # (the shapes the issue names: X = 16 takes k_edt_y4 since that kernel exists; Y > 512 at X % 4 != 0 takes k_edt_y<32,16>)
    ((16, 1024, 12), 0, False, F.NONE, {"k_edt_y4<32>", "k_edt_x<1>", "k_edt_z_direct", "k_edt_z<1,16,8>"}),
    ((3, 1024, 2), 0, False, F.NONE, {"k_edt_y<32,16>", "k_edt_x<1>", "k_edt_z_direct", "k_edt_z<1,16,8>"}),
    ((2, 300, 2), 0, False, F.NONE, {"k_edt_y<16,16>", "k_edt_x<1>", "k_edt_z_direct", "k_edt_z<1,16,8>"}),
    ((5, 256, 3), 0, True, F.NONE, {"k_edt_z<1,16,8>"}),
    ((130, 16, 176), 0, False, F.NONE, {"k_edt_y<8,8>", "k_edt_x<4>", "k_edt_z_stream<true>", "k_edt_x_redo<4>", "k_edt_z<4,16,8>"}),
    ((130, 16, 176), 1, True, F.NONE, {"k_edt_z_stream<true>", "k_edt_x_redo<4>", "k_edt_z<4,16,8>"}),
    ((129, 16, 176), 0, False, F.NONE, {"k_edt_y<8,8>", "k_edt_x<4>", "k_edt_z_stream<false>", "k_edt_z<4,16,8>"}),
    ((129, 16, 176), 1, True, F.NONE, {"k_edt_z_stream<false>", "k_edt_z<4,16,8>"}),
    ((12, 12, 1024), 1, False, F.NONE, {"k_edt_y4<16>", "k_edt_x<1>", "k_edt_z_stream<true>", "k_edt_x_redo<1>", "k_edt_z<16,16,8>"}),
    ((1024, 6, 11), 0, False, F.NONE, {"k_edt_y4<16>", "k_edt_x<16>", "k_edt_z_direct", "k_edt_z<1,16,8>"}),
    ((514, 56, 2), 0, False, F.NONE, {"k_edt_y<8,8>", "k_edt_x<16>", "k_edt_z_direct", "k_edt_z<1,16,8>"}),
    # the guesses, read off the table of DESIGN.md 31 ("the hint"): "took" launches no pass X; "left" the streaming form that reads
    # pass X's planes and no k_edt_x_redo; neither counts where the fused form cannot take the volume (odd X, Z < 64) or for a completion
    ((130, 16, 176), 0, False, F.TOOK, {"k_edt_y<8,8>", "k_edt_z_stream<true>", "k_edt_x_redo<4>", "k_edt_z<4,16,8>"}),
    ((130, 16, 176), 0, False, F.LEFT, {"k_edt_y<8,8>", "k_edt_x<4>", "k_edt_z_stream<false>", "k_edt_z<4,16,8>"}),
    ((129, 16, 176), 0, False, F.TOOK, {"k_edt_y<8,8>", "k_edt_x<4>", "k_edt_z_stream<false>", "k_edt_z<4,16,8>"}),
    ((129, 16, 176), 0, False, F.LEFT, {"k_edt_y<8,8>", "k_edt_x<4>", "k_edt_z_stream<false>", "k_edt_z<4,16,8>"}),
    ((130, 16, 176), 1, True, F.TOOK, {"k_edt_z_stream<true>", "k_edt_x_redo<4>", "k_edt_z<4,16,8>"}),
    ((130, 16, 176), 1, True, F.LEFT, {"k_edt_z_stream<true>", "k_edt_x_redo<4>", "k_edt_z<4,16,8>"}),
    ((16, 1024, 12), 0, False, F.TOOK, {"k_edt_y4<32>", "k_edt_x<1>", "k_edt_z_direct", "k_edt_z<1,16,8>"}),
    ((12, 12, 1024), 1, False, F.TOOK, {"k_edt_y4<16>", "k_edt_z_stream<true>", "k_edt_x_redo<1>", "k_edt_z<16,16,8>"}),
]
# (the rows without a guess keep the ids they had before the guess was a column)
HAND_IDS = ["size%d-%d-%s-" % (i, r[1], r[2]) + ("" if r[3] == F.NONE else "guess%d-" % r[3]) + "want%d" % i for i, r in enumerate(HAND_ROWS)]


@pytest.mark.parametrize("size,full,completion,guess,want", HAND_ROWS, ids=HAND_IDS)
def test_host_forms_by_hand(size, full, completion, guess, want):
    """the launch rules, read off gie_edt_plan_for (what be_edt / be_edt_z execute) by hand for a few shapes"""
    assert F.host_forms(size, 1, 1, full, completion, guess) == want
    assert F.host_forms(size, 500, 10 ** 6, full, completion, guess) == want     # (the counts change no launch)
    if guess == F.NONE:
        assert F.host_forms(size, 1, 1, full, completion) == want                # (a fresh mapper's guess is NONE)


def test_the_device_rules_at_their_borders():
    # 160 / 161 sites; 8 kall = 7 X and one site fewer (X = 256: 224 / 223)
    for k, want in ((1, "banded"), (160, "banded"), (161, "dnc"), (223, "dnc"), (224, "windowed"), (256, "windowed")):
        occ = np.zeros((1, 4, 256), bool)
        occ[0, 1, F.spread(256, k)] = True
        form, clear = F.row_forms_x(occ)
        assert set(form[0]) == {want} and clear.all(), (k, form[0])
    # the window's reach: a row 48 from its sites is let go (48^2 < 49^2), a row 49 away is not; neither is clear
    occ = np.zeros((1, 50, 256), bool)
    occ[0, 0, :] = True
    form, clear = F.row_forms_x(occ)
    assert form[0, 48] == "windowed" and form[0, 49] == "gives_up" and not clear[0, 48] and not clear[0, 49]
    assert form[0, 46] == "windowed" and clear[0, 46]
    # planes with obstacles: 160 banded, 161 the window (CP >= 4); the streaming form takes 161 where Z >= 64
    assert F.z_worker((12, 12, 256), 160, 0, 1) == "column" and F.z_worker((12, 12, 256), 161, 0, 1) == "stream"
    assert F.z_worker((12, 12, 63), 63, 0, 1) == "column"
    # the list form: short volumes always, otherwise up to an eighth of the tiles; GIE_TILE_LIST forces either
    assert F.z_worker((40, 24, 40), 20, 15, 0) == "list" and F.z_worker((40, 24, 40), 20, 15, 0, 0) == "column"
    assert F.z_worker((40, 24, 72), 36, 16, 0) == "list" and F.z_worker((40, 24, 72), 36, 17, 0) == "column"      # 135 tiles
    assert F.z_worker((24, 24, 256), 186, 200, 0) == "stream" and F.z_worker((24, 24, 256), 186, 200, 0, 1) == "list"
    assert F.stream_segments((130, 16, 176)) == (2, 96)                   # two z segments of unequal length: 96 and 80 planes


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_claims_and_its_expectation_is_right(oracle_lib, name):
    c = F.case(name)
    X, Y, Z = c.size
    assert X * Y * Z <= 1500000
    occ = c.occ()
    assert occ.any()
    got = F.derived_coverage(c, occ)
    assert sorted(c.covers - got, key=str) == [], "claims that do not follow from the obstacles"
    if c.partial and c.conditions:
        lab = c.labels()
        assert lab.shape == (Z, Y, X) and set(np.unique(lab)) <= {0, 1, 2}
        cond = F.partial_conditions(c.size, F.need_of_labels(lab))
        assert all(cond.values()), cond
        assert ("a band without a reader between two with one" in cond) == (F.cp_of(Z) >= 4)
    # the reference side: the oracle's EDT alone against the closed form (distances and closest obstacles, tie rule included)
    # and against the definition
    d, coc = F.expected(name)
    rd, rc = tie_rule_reference(occ)
    assert np.array_equal(d, rd)
    assert np.array_equal(coc, rc)
    if X * Y * Z <= 300000:
        assert np.array_equal(d, brute_force_edt(occ.astype(np.int8)))


def test_pass_y_patterns_are_the_edges_they_are_named_for():
    for X, Y in ((5, 256), (7, 513), (4, 16), (68, 513)):
        kern, share = F.pass_y_kernel(X, Y)
        p = {n: np.nonzero(F.y_pattern(n, Y, share))[0] for n in F.Y_PATTERNS}
        assert p["empty"].size == 0 and p["full"].size == Y
        assert list(p["y0"]) == [0] and list(p["ylast"]) == [Y - 1]
        if Y > 32:
            assert all(k - 1 in p["word_borders"] and k in p["word_borders"] for k in range(32, Y, 32))
        if Y > share:
            assert share - 1 in p["share_borders"] and share in p["share_borders"]
        gaps = np.diff(p["even_pairs"])
        assert gaps.size and (gaps % 2 == 0).all()                        # every midpoint ties
        if Y > 520:
            assert np.diff(p["long_gap"]).max() > 512
        vol = F.y_pattern_volume(X, Y)
        assert not vol[-1].any() and F.y_patterns_present(vol) == set(F.Y_PATTERNS)
        # an empty column stands between two full ones
        cols = [vol[z, :, x] for z in range(vol.shape[0] - 1) for x in range(X)]
        assert cols[0].all() and not cols[1].any() and cols[2].all()
