"""CPU: the placement case tables of tests/gemm_placement.py reach every dispatch branch of the matrix-product
exports, and every placement a MSAT_REQUIRE forbids is refused before anything is launched (dummy non-null
pointers, never dereferenced)."""
import pytest

import gemm_placement as gp

A16 = 0x10000  # a 16-byte aligned dummy address


@pytest.mark.parametrize("export", sorted(gp.TABLES))
def test_case_table_reaches_every_branch(export):
    got = {gp.expected_path(export, c) for c in gp.TABLES[export]}
    assert got == set(gp.BRANCHES[export]), (sorted(set(gp.BRANCHES[export]) - got), sorted(got - set(gp.BRANCHES[export])))
    names = [c.name for c in gp.TABLES[export]]
    assert len(names) == len(set(names)), "duplicate case names"


def test_branch_lists_name_what_the_issue_names():
    flat = {b for v in gp.BRANCHES.values() for b in v}
    for part in ("x3w", "x3_tiles", "wgrad2", "wgrad_generic"):
        for red in ("reduce4", "reduce_scalar"):
            assert f"{part}/{red}" in flat
    assert {"gemm2/vec", "gemm2/scalar", "gemm_kernel", "skinny/av", "skinny/scalarA", "two_range"} <= flat


def test_two_range_fallback_reaches_fast_and_generic_subproducts():
    sub = set()
    for c in gp.WGRAD_ROT_CASES:
        if gp.expected_path("msat_gemm_wgrad_rot", c) == "two_range":
            sub |= set(gp.two_range_subpaths(c))
    assert set(gp.TWO_RANGE_SUBPATHS) <= sub, sorted(set(gp.TWO_RANGE_SUBPATHS) - sub)


def test_pair_tables_differ_only_in_the_epilogue():
    """The bitwise pairs: same partial kernel / main loop on both sides, the float4 epilogue on one and the
    scalar one on the other."""
    by = {c.name: c for c in gp.GEMM_CASES}
    for v, s in gp.GEMM_VEC_SCALAR_PAIRS:
        assert gp.expected_path("msat_gemm", by[v]) == "gemm2/vec"
        assert gp.expected_path("msat_gemm", by[s]) == "gemm2/scalar"
        assert (by[v].a, by[v].b) == (by[s].a, by[s].b)
    by = {c.name: c for c in gp.WGRAD_CASES}
    parts = set()
    for v, s in gp.WGRAD_REDUCE_PAIRS:
        pv, ps = gp.expected_path("msat_gemm_wgrad", by[v]), gp.expected_path("msat_gemm_wgrad", by[s])
        assert pv.endswith("/reduce4") and ps.endswith("/reduce_scalar") and pv.split("/")[0] == ps.split("/")[0]
        parts.add(pv.split("/")[0])
    assert parts == {"x3w", "x3_tiles", "wgrad2"}
    assert {gp.expected_path("msat_gemm", c) for c in gp.GEMM_ACC2_CASES} == set(gp.BRANCHES["msat_gemm"])


def _refused(rc, msg):
    from marlsat import _lib

    assert rc == -1
    assert msg in _lib.lib.msat_last_error().decode()


X3_MSG = "gemm_x3: K % 16, lda % 4 and 16-byte aligned operands required"
H2_MSG = "gemm_h2: K % 32, lda % 4 and 16-byte aligned operands required"


@pytest.mark.parametrize("bad", [dict(lda=50), dict(A=A16 + 4), dict(planes=A16 + 8), dict(ldc=124), dict(K=40, lda=40),
                                 dict(K=8, lda=8), dict(lda=44)])
def test_gemm_x3_refusals(bad):
    from marlsat import _lib

    a = dict(A=A16, lda=48, planes=A16, C=A16, ldc=128, bias=A16, M=5, N=128, K=48)
    a.update(bad)
    _refused(_lib.lib.msat_gemm_x3(a["A"], a["lda"], a["planes"], a["C"], a["ldc"], a["bias"], a["M"], a["N"], a["K"],
                                   0, None), X3_MSG)


@pytest.mark.parametrize("bad", [dict(lda=98), dict(A=A16 + 4), dict(p2=A16 + 2), dict(p3=A16 + 8), dict(ldc=127),
                                 dict(K=48, lda=48), dict(K=80, lda=96), dict(lda=92)])
def test_gemm_h2_refusals(bad):
    from marlsat import _lib

    a = dict(A=A16, lda=96, p2=A16, p3=A16, C=A16, ldc=128, M=5, N=128, K=96)
    a.update(bad)
    _refused(_lib.lib.msat_gemm_h2(a["A"], a["lda"], A16, a["p2"], a["p3"], A16, a["C"], a["ldc"], None, a["M"],
                                   a["N"], a["K"], 0, None), H2_MSG)


@pytest.mark.parametrize("bad", [dict(lda0=514), dict(lda1=510), dict(A0=A16 + 4), dict(A1=A16 + 12), dict(W0h=A16 + 8),
                                 dict(W1x=A16 + 2), dict(ldc0=127), dict(ldc1=100), dict(K=400), dict(lda0=380)])
def test_gemm_h2_dual_refusals(bad):
    from marlsat import _lib

    a = dict(A0=A16, lda0=512, W0h=A16, W0x=A16, C0=A16, ldc0=128, N0=128, A1=A16, lda1=512, W1h=A16, W1x=A16,
             C1=A16, ldc1=128, N1=128, M=5, K=384)
    a.update(bad)
    rc = _lib.lib.msat_gemm_h2_dual(a["A0"], a["lda0"], a["W0h"], a["W0x"], A16, a["C0"], a["ldc0"], a["N0"], 1,
                                    a["A1"], a["lda1"], a["W1h"], a["W1x"], A16, a["C1"], a["ldc1"], a["N1"], 0, A16,
                                    a["M"], a["K"], None)
    _refused(rc, "gemm_h2_dual: K % 32, lda % 4 (planes: % 8) and 16-byte aligned operands required")


WH2_ALIGN = "gemm_wgrad_h2: K % 4, N % 4, ld % 4 and 16-byte aligned operands required"


@pytest.mark.parametrize("bad,msg", [
    (dict(K=18, lda=20), WH2_ALIGN), (dict(N=130, ldg=132, ldw=132), WH2_ALIGN), (dict(lda=17), WH2_ALIGN),
    (dict(ldg=129), WH2_ALIGN), (dict(A=A16 + 4), WH2_ALIGN), (dict(G=A16 + 8), WH2_ALIGN), (dict(ws=A16 + 4), WH2_ALIGN),
    (dict(rot=6), "gemm_wgrad_h2: rot must be in [0, N), a multiple of 4"),
    (dict(rot=128), "gemm_wgrad_h2: rot must be in [0, N), a multiple of 4"),
    (dict(lda=12), "gemm_wgrad_h2: bad dims"), (dict(ldg=124), "gemm_wgrad_h2: bad dims"),
    (dict(ldw=127), "gemm_wgrad_h2: bad dims"), (dict(K=8, lda=8), "gemm_wgrad_h2: bad dims"),
    (dict(N=388, ldg=388, ldw=388), "gemm_wgrad_h2: bad dims"),
])
def test_gemm_wgrad_h2_refusals(bad, msg):
    from marlsat import _lib

    a = dict(A=A16, lda=16, G=A16, ldg=128, W=A16, ldw=128, M=5, K=16, N=128, rot=4, ws=A16)
    a.update(bad)
    _refused(_lib.lib.msat_gemm_wgrad_h2(a["A"], a["lda"], a["G"], a["ldg"], A16, a["W"], a["ldw"], a["M"], a["K"],
                                         a["N"], a["rot"], 0, a["ws"], None), msg)


DUAL_ALIGN = "gemm_wgrad_h2_dual: K % 4, N % 4, ld % 4 and 16-byte aligned operands required"
PLANES_MSG = "gemm_wgrad_h2_dual_planes: K % 4, N % 8, lda % 4, ldg % 8, plo % 8"


def _dual_args(bad):
    a = dict(A0=A16, lda0=128, G0=A16, ldg0=512, W0=A16, ldw0=384, K0=128, N0=384, rot0=0,
             A1=A16, lda1=256, G1=A16, ldg1=512, W1=A16, ldw1=384, K1=256, N1=384, rot1=256, M=5, ws=A16)
    a.update(bad)
    return a


@pytest.mark.parametrize("bad,msg", [
    (dict(K0=18, lda0=20), DUAL_ALIGN), (dict(K1=254), DUAL_ALIGN), (dict(N0=382), DUAL_ALIGN), (dict(N1=130, rot1=0), DUAL_ALIGN),
    (dict(lda0=129), DUAL_ALIGN), (dict(lda1=258), DUAL_ALIGN), (dict(ldg0=513), DUAL_ALIGN), (dict(ldg1=514), DUAL_ALIGN),
    (dict(A0=A16 + 4), DUAL_ALIGN), (dict(A1=A16 + 8), DUAL_ALIGN), (dict(G0=A16 + 4), DUAL_ALIGN),
    (dict(G1=A16 + 12), DUAL_ALIGN), (dict(ws=A16 + 4), "gemm_wgrad_h2_dual: workspace alignment"),
    (dict(rot0=6), "gemm_wgrad_h2_dual: bad rot"), (dict(rot1=384), "gemm_wgrad_h2_dual: bad rot"),
    (dict(ldw0=380), "gemm_wgrad_h2_dual: bad dims"), (dict(lda1=252), "gemm_wgrad_h2_dual: bad dims"),
    (dict(ldg0=380), "gemm_wgrad_h2_dual: bad dims"),
])
def test_gemm_wgrad_h2_dual_refusals(bad, msg):
    from marlsat import _lib

    a = _dual_args(bad)
    rc = _lib.lib.msat_gemm_wgrad_h2_dual(a["A0"], a["lda0"], a["G0"], a["ldg0"], a["W0"], a["ldw0"], a["K0"], a["N0"],
                                          a["rot0"], a["A1"], a["lda1"], a["G1"], a["ldg1"], a["W1"], a["ldw1"],
                                          a["K1"], a["N1"], a["rot1"], A16, a["M"], 0, a["ws"], None)
    _refused(rc, msg)


@pytest.mark.parametrize("bad,msg", [
    (dict(K0=18, lda0=20), PLANES_MSG), (dict(N1=380), PLANES_MSG), (dict(lda0=130), PLANES_MSG), (dict(ldg0=1028), PLANES_MSG),
    (dict(ldg1=1020), PLANES_MSG), (dict(plo=516), PLANES_MSG), (dict(plo=376), PLANES_MSG), (dict(plo=648), PLANES_MSG),
    (dict(A1=A16 + 4), PLANES_MSG), (dict(G0=A16 + 8), PLANES_MSG), (dict(G1=A16 + 2), PLANES_MSG),
    (dict(ws=A16 + 4), "gemm_wgrad_h2_dual: workspace alignment"), (dict(rot1=6), "gemm_wgrad_h2_dual: bad rot"),
])
def test_gemm_wgrad_h2_dual_planes_refusals(bad, msg):
    """The planes form: ldg in fp16 elements (1024 = [hi 4H | lo 4H]), the lo plane plo elements after hi."""
    from marlsat import _lib

    a = _dual_args(dict(ldg0=1024, ldg1=1024, plo=512))
    a.update(bad)
    rc = _lib.lib.msat_gemm_wgrad_h2_dual_planes(a["A0"], a["lda0"], a["G0"], a["ldg0"], a["W0"], a["ldw0"], a["K0"],
                                                 a["N0"], a["rot0"], a["A1"], a["lda1"], a["G1"], a["ldg1"], a["W1"],
                                                 a["ldw1"], a["K1"], a["N1"], a["rot1"], a["plo"], A16, a["M"], 0,
                                                 a["ws"], None)
    _refused(rc, msg)


@pytest.mark.parametrize("bad", [dict(lda=31), dict(ldc=129), dict(ldb=31, transB=1), dict(ldb=129, transB=0)])
def test_gemm_leading_dims_refused(bad):
    from marlsat import _lib

    a = dict(lda=32, ldb=32, transB=1, ldc=130)
    a.update({"ldb": 130} if bad.get("transB") == 0 else {})
    a.update(bad)
    _refused(_lib.lib.msat_gemm(A16, a["lda"], A16, a["ldb"], a["transB"], A16, a["ldc"], None, 5, 130, 32, 0, None),
             "leading dims too small")


@pytest.mark.parametrize("rot", [None, 0, 4])
@pytest.mark.parametrize("bad", [dict(lda=15), dict(ldg=7), dict(ldw=7)])
def test_wgrad_leading_dims_refused(bad, rot):
    from marlsat import _lib

    a = dict(lda=16, ldg=8, ldw=8)
    a.update(bad)
    if rot is None:
        rc = _lib.lib.msat_gemm_wgrad(A16, a["lda"], A16, a["ldg"], A16, a["ldw"], 5, 16, 8, 0, A16, None)
    else:
        rc = _lib.lib.msat_gemm_wgrad_rot(A16, a["lda"], A16, a["ldg"], A16, a["ldw"], 5, 16, 8, rot, 0, A16, None)
    _refused(rc, "bad dims")


def test_wgrad_rot_range_refused():
    from marlsat import _lib

    for rot in (-1, 8):
        _refused(_lib.lib.msat_gemm_wgrad_rot(A16, 16, A16, 8, A16, 8, 5, 16, 8, rot, 0, A16, None),
                 "gemm_wgrad_rot: rot must be in [0, N)")
