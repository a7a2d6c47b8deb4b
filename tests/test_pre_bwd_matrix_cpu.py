"""CPU companion of tests/test_gpu_pre_bwd_matrix.py: keeps its case table honest.

1. A restatement of the dispatch rule of the per-Gaussian backward (csrc/api.hip, `backward_impl`'s lookup in
   `hgs_pre_bwd_forms`; csrc/preprocess.hip: the rows of `HGS_PRE_BWD_FORMS`, `sh_block_vectorisable`, `hgs_sh_staged`,
   the `staged` condition of `preprocess_bwd_body`) applied to the table: every launch target, every SH path a target can
   take, with M == NC and M > NC, and every listed boundary must be hit; a failure names what is missing.  The form table
   has 24 slots that are 23 kernels: the loop form at SH degree 3 (`d3`) serves the filter through a run-time bit
   ("d3+aa" below).  The expectation is for a device that grants the 160 KB dynamic-LDS raise (MI355X).
2. The condition behind the GPU module's gate (1e-3 of max|g64|): on every distinct scene of the table (the filter
   included), for every view and for every sum over views the table uses, the fp32 ORACLE is within a quarter of it, and
   at least 90 % of the Gaussians are visible in at least one view.  A condition on the inputs, checked on the reference
   alone: the oracle's fp32 run is typically 3e-6 from its fp64 run on these scenes; a (scene, view) where it is not holds
   a hard decision of the blend (alpha >= 1/255, the filter's clamp) that fp32 and fp64 take differently - there ANY fp32
   implementation steps away from fp64 by a finite amount, and the scene's seed has to change, not the gate."""
import pytest
import torch

import test_gpu_pre_bwd_matrix as T

ALLOWED_M = {0: (1, 16), 1: (4, 5, 10, 16, 25), 2: (9, 10, 13, 16), 3: (16, 25)}     # SH storage per active degree
DEFAULT_TARGETS = ([f"{f}{d}{a}" for f in "sp" for d in range(4) for a in ("", "_aa")]
                   + ["d2", "d3", "d2_aa", "d3+aa"])
LOOP_BUILD_TARGETS = ["d0", "d1", "d0_aa", "d1_aa"]       # reachable only when HGS_PRE_BWD_VPAR_MIN_VIEWS > HGS_MAX_VIEWS


def target(c, loop_build=False):
    """the kernel api.hip launches for the case (loop_build: the second build of the GPU module)"""
    deg = c.deg if c.color == "sh" else 0
    lds = (23 + 3 * (deg + 1) ** 2) * 64 * c.B * 4
    vpar = not loop_build and 2 <= c.B <= (8 if deg >= 2 else 16) and lds <= 160 * 1024
    form = "s" if c.B == 1 else ("p" if vpar else "d")
    return f"{form}{deg}" + (("+aa" if (form, deg) == ("d", 3) else "_aa") if c.aa else "")


def sh_paths(form, deg, M, P, packed):
    """how the (M, 3) gradient block of a Gaussian leaves the kernel"""
    if M == 0:
        return set()
    if packed:
        return {"packed"}
    direct = "vector" if (3 * M) % 4 == 0 and M <= 16 else "scalar"
    staged = form == "s" and deg > 0 and 4 <= M <= 16              # full 256-chunks only
    return ({"staged"} if staged and P >= 256 else set()) | ({direct} if not staged or P % 256 else set())


def coverage(loop_build):
    hit = set()
    for c in (T.MULTI_VIEW_CASES if loop_build else T.CASES):
        t = target(c, loop_build)
        runs = [c.out == "packed"] + ([False] if c.out == "packed" and not loop_build else [])   # (+ the six-tensor companion run)
        for packed in runs:
            for p in sh_paths(t[0], c.deg, c.M, c.P, packed):
                hit.add((t, p, c.M > T.nc_of(c.deg)))
        hit.add((t, None, None))
    return hit


def required(targets):
    need = set()
    for t in targets:
        deg = int(t[1])
        need.add((t, None, None))
        for M in ALLOWED_M[deg]:
            for packed in (False, True):
                for P in (255, 256, 257):
                    for p in sh_paths(t[0], deg, M, P, packed):
                        need.add((t, p, M > T.nc_of(deg)))
    return need


def test_the_table_reaches_every_kernel_and_sh_path():
    assert len(DEFAULT_TARGETS) == 20 and len(LOOP_BUILD_TARGETS) == 4
    assert len({t.replace("+aa", "") for t in DEFAULT_TARGETS + LOOP_BUILD_TARGETS}) == 23         # distinct kernels
    missing = sorted(map(str, required(DEFAULT_TARGETS) - coverage(False)))
    assert not missing, ("default build: (kernel, SH path, M > NC) without a case", missing)
    missing = sorted(map(str, required(LOOP_BUILD_TARGETS + ["d2", "d3", "d2_aa", "d3+aa"]) - coverage(True)))
    assert not missing, ("loop-form build: (kernel, SH path, M > NC) without a case", missing)
    assert {t for t, _, _ in coverage(True)} == set(LOOP_BUILD_TARGETS + ["d2", "d3", "d2_aa", "d3+aa"])
    assert {t for t, _, _ in coverage(False)} == set(DEFAULT_TARGETS)


def test_the_table_holds_every_boundary():
    C = T.CASES
    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)
    need("views", {c.B for c in C} == {1, 2, 3, 8, 9, 16})
    need("one-view P", {c.P for c in C if c.B == 1} == {1, 63, 255, 256, 257, 577})
    need("multi-view P", {c.P for c in C if c.B > 1} == {63, 64, 65, 577})
    for deg in range(4):
        need(f"M at degree {deg}", {c.M for c in C if c.deg == deg and c.color == "sh"} == set(ALLOWED_M[deg]))
        for aa in (False, True):
            need(f"degree {deg}, filter {aa}: M > NC and M == NC, one view and many",
                 {(c.B > 1, c.M > T.nc_of(deg)) for c in C if c.deg == deg and c.aa == aa and c.color == "sh"}
                 == {(False, False), (False, True), (True, False), (True, True)})
            if deg <= 1:       # 16 views in the thread-per-(Gaussian, view) form: more than 64 KB of LDS
                need(f"16 views at degree {deg}, filter {aa}", any(c.B == 16 and c.deg == deg and c.aa == aa and c.color == "sh" for c in C))
            else:              # 8 -> 9 views: the form switch
                need(f"8 and 9 views at degree {deg}, filter {aa}",
                     {8, 9} <= {c.B for c in C if c.deg == deg and c.aa == aa})
    for aa in (False, True):
        for many in (False, True):
            sel = [c for c in C if c.aa == aa and (c.B > 1) == many]
            need(f"colors_precomp (filter {aa}, many views {many})", any(c.color == "precomp" for c in sel))
            need(f"cov3D_precomp (filter {aa}, many views {many})", any(c.cov == "cov" for c in sel))
            need(f"scale_modifier 0.7 (filter {aa}, many views {many})", any(c.mod == 0.7 for c in sel))
            need(f"fused, six tensors and packed (filter {aa}, many views {many})", {c.out for c in sel if c.fused} == {"six", "packed"})
            need(f"packed, M > NC (filter {aa}, many views {many})", any(c.out == "packed" and c.M > T.nc_of(c.deg) for c in sel))
    # the two staged chunks + a tail of one launch, staged and not vectorisable
    need("P = 577 staged with M not a multiple of 4", any(c.B == 1 and c.P == 577 and c.M in (5, 10, 13) and c.out == "six" for c in C))
    need("M > 16", any(c.M == 25 and c.B == 1 for c in C) and any(c.M == 25 and c.B > 1 for c in C))
    assert all(c.M >= T.nc_of(c.deg) for c in C if c.color == "sh") and all(c.deg == 0 for c in C if c.color == "precomp")
    assert len(set(C)) == len(C)
    assert not missing, missing


# ------------------------------------------------------------------------------------------------- the condition behind the gate
ORACLE_TOL = 0.25 * T.GRAD_TOL


def _scene_key(c):
    return T.ref_key(c, 0)[:-1]


def _distinct_scenes():
    seen = {}
    for c in T.CASES:
        key = _scene_key(c)
        seen[key] = max(seen.get(key, 0), c.B)
    return sorted(seen.items(), key=str)


def _check(g32, g64, visible, what):
    for k in g64:
        scale = max(float(g64[k].abs().max()), 1e-300)
        err = float((g32[k] - g64[k]).abs().max()) / scale
        assert err <= ORACLE_TOL, (what, k, err)
    assert float(visible.float().mean()) >= 0.9, (what, float(visible.float().mean()))


@pytest.mark.parametrize("key,views", _distinct_scenes(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_fp32_oracle_is_within_a_quarter_of_the_gate(key, views):
    """per distinct scene, for every number of views the table uses on it: gradients summed over the views"""
    deg, P, aa, color, cov, mod = key
    used = sorted({c.B for c in T.CASES if _scene_key(c) == key})
    assert used[-1] == views
    for B in used:
        c = T._c(B, deg, aa, T.nc_of(deg), P, color=color, cov=cov, mod=mod)
        (g32, _), (g64, visible) = T.reference(c, torch.float32), T.reference(c, torch.float64)
        _check(g32, g64, visible, (key, B))
    for b in range(views):
        (g32, _), (g64, _) = T.reference_view(c, b, torch.float32), T.reference_view(c, b, torch.float64)
        _check(g32, g64, torch.ones(1), (key, "view", b))


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_the_reference_gives_the_inactive_coefficients_no_gradient(deg):
    """what the GPU module asserts bitwise: with M = 25 stored coefficients the oracle's gradient beyond (D+1)^2 is exactly 0"""
    c = T._c(1, deg, False, 25, 63)
    sc = T.scene(deg, 63)
    out = T.oracle.forward_backward(sc["means3D"], sc["shs"], None, sc["opacities"], sc["scales"], sc["rotations"], None,
                                    T._oracle_settings(c, 0), *T.upstream(0), dtype=torch.float64)
    g = out["grads"]["shs"]
    assert g.shape == (63, 25, 3) and float(g[:, :T.nc_of(deg)].abs().max()) > 0
    assert float(g[:, T.nc_of(deg):].abs().max()) == 0.0


@pytest.mark.parametrize("aa", [False, True], ids=["off", "aa"])
def test_the_fp32_oracle_on_the_edge_scene(aa):
    for B in (1, 3):
        g32, g64 = T.edge_reference(B, aa, torch.float32), T.edge_reference(B, aa, torch.float64)
        dead = T.rows_without_reference_gradient(g64, T.EDGE_P)
        _check(g32, g64, ~dead, ("edge", aa, B))
    raw = T.edge_raw()
    assert int((dead & (raw["opacities"].reshape(-1) <= -12)).sum()) == 12
    assert float(raw["scales"].min()) == -9.0 and float(raw["scales"].max()) == 0.0
    n = raw["rotations"].norm(dim=1)
    assert float(n.min()) < 1.1e-3 and float(n.max()) > 0.9e3
    assert {float(v) for v in raw["opacities"].reshape(-1) if abs(float(v)) >= 12} == {12.0, -12.0, 30.0, -30.0}
