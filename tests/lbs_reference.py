"""numpy restatement of linear blend skinning as include/hgs_rast.h (hgs_lbs_pose) states it - [UPSTREAM-KNOWLEDGE] the
`smplx` package's lbs() with its batch_rodrigues - with a dtype switch:

  float64   the reference the GPU tests measure against;
  float32   every operation rounded to fp32, 3-term dot products as (a0 b0 + a1 b1) + a2 b2, the sum over the K pose-blend
            rows and the sum over the joints each accumulated in index order.  Its own distance to float64 is the unit the
            GPU gate is expressed in (the kernel partitions the K-sum, so it is not bit-equal to this form).

Also: the seeded synthetic bodies and the table of cases the boundary sweep runs (tests/test_gpu_lbs.py on the device,
tests/test_lbs_cpu.py for the fp32 form alone, so that the GPU gate is not vacuous)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23

# [UPSTREAM-KNOWLEDGE] kintree_table[0] of the SMPL-X model file (55 joints: 22 body, jaw, two eyes, 2 x 15 fingers)
SMPLX_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53)


def parents_of(tree, J):
    """chain: depth J - 1; star: every joint hangs on the root; smplx: the SMPL-X table (cut at J, continued as a chain)"""
    if tree == "chain":
        return np.arange(-1, J - 1, dtype=np.int32)
    if tree == "star":
        return np.array([-1] + [0] * (J - 1), dtype=np.int32)
    if tree == "smplx":
        return np.array([SMPLX_PARENTS[j] if j < len(SMPLX_PARENTS) else j - 1 for j in range(J)], dtype=np.int32)
    raise ValueError(tree)


def make_body(V, J, tree="smplx", width=4, pose_blend=True, seed=0, num_shape=3, mesh=None):
    """A seeded synthetic body: fp32 arrays in the lbs layout.  weights (V, J) dense, positive on 1..width joints per vertex
    (vertex 0 on exactly `width`), rows summing to 1; posedirs (9 (J - 1), 3 V) or None; shapedirs (V, 3, num_shape).
    mesh = (vertices, faces): the template is that mesh (V is its vertex count) instead of random points."""
    rng = np.random.default_rng(seed)
    width = min(width, J)
    v_template = rng.uniform(-1.0, 1.0, (V, 3)).astype(np.float32)
    if mesh is not None:
        v_template = np.asarray(mesh[0], np.float32)
        assert v_template.shape == (V, 3)
    reg = rng.uniform(0.0, 1.0, (J, V)) ** 4
    J_regressor = (reg / reg.sum(1, keepdims=True)).astype(np.float32)
    weights = np.zeros((V, J), np.float64)
    for v in range(V):
        n = width if v == 0 else int(rng.integers(1, width + 1))
        idx = rng.choice(J, size=n, replace=False)
        weights[v, idx] = rng.uniform(0.05, 1.0, n)
    weights = (weights / weights.sum(1, keepdims=True)).astype(np.float32)
    K = 9 * (J - 1) if pose_blend else 0
    posedirs = (rng.standard_normal((K, 3 * V)) * 0.01).astype(np.float32) if K else None
    shapedirs = (rng.standard_normal((V, 3, num_shape)) * 0.03).astype(np.float32)
    faces = np.stack([np.arange(V), (np.arange(V) + 1) % V, (np.arange(V) + 2) % V], 1).astype(np.int32)
    if mesh is not None:
        faces = np.asarray(mesh[1], np.int32)
    return dict(v_template=v_template, faces=faces, parents=parents_of(tree, J), J_regressor=J_regressor, weights=weights,
                shapedirs=shapedirs, posedirs=posedirs)


def setup(body, betas=None):
    """the once-per-body part, in float64: v_shaped (V, 3) and J_rest (J, 3)"""
    v = body["v_template"].astype(np.float64)
    if betas is not None and body.get("shapedirs") is not None:
        b = np.asarray(betas, np.float64)
        v = v + body["shapedirs"].astype(np.float64)[:, :, :b.size] @ b
    return v, body["J_regressor"].astype(np.float64) @ v


def _mm3(A, B):
    return np.stack([np.stack([(A[..., r, 0] * B[..., 0, c] + A[..., r, 1] * B[..., 1, c]) + A[..., r, 2] * B[..., 2, c]
                               for c in range(3)], -1) for r in range(3)], -2)


def _mv3(A, x):
    return np.stack([(A[..., r, 0] * x[..., 0] + A[..., r, 1] * x[..., 1]) + A[..., r, 2] * x[..., 2] for r in range(3)], -1)


def rodrigues(a, dtype=np.float64):
    """(..., 3) axis-angle -> (..., 3, 3): angle = |a + 1e-8|, k = a / angle, R = I + sin [k]x + (1 - cos) [k]x^2"""
    dt = np.dtype(dtype).type
    a = np.asarray(a).astype(dt)
    b = a + dt(1e-8)
    angle = np.sqrt((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2])
    k = a / angle[..., None]
    s, oc = np.sin(angle)[..., None, None], (dt(1.0) - np.cos(angle))[..., None, None]
    Kx = np.zeros(a.shape[:-1] + (3, 3), dt)
    Kx[..., 0, 1], Kx[..., 0, 2] = -k[..., 2], k[..., 1]
    Kx[..., 1, 0], Kx[..., 1, 2] = k[..., 2], -k[..., 0]
    Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 1], k[..., 0]
    R = (np.eye(3, dtype=dt) + s * Kx) + oc * _mm3(Kx, Kx)
    assert R.dtype == dt
    return R


def pose(v_shaped, J_rest, parents, weights, posedirs, poses, transl=None, centre=None, scale=1.0, dtype=np.float64):
    """poses (F, J, 3) -> (vertices (F, V, 3), joints (F, J, 3)) in `dtype`; inputs are cast to it first (v_shaped and J_rest
    are the float64 set-up: the float32 form starts from their fp32 casts, as the device does)."""
    dt = np.dtype(dtype).type
    v_shaped, J_rest = np.asarray(v_shaped).astype(dt), np.asarray(J_rest).astype(dt)
    weights, poses = np.asarray(weights).astype(dt), np.asarray(poses).astype(dt)
    F, J = poses.shape[:2]
    V = v_shaped.shape[0]
    R = rodrigues(poses, dt)                                                  # (F, J, 3, 3)
    acc = np.zeros((F, 3 * V), dt)
    if posedirs is not None and len(posedirs):
        pd = np.asarray(posedirs).astype(dt)
        pf = (R[:, 1:] - np.eye(3, dtype=dt)).reshape(F, -1)
        assert pd.shape == (pf.shape[1], 3 * V)
        for k in range(pd.shape[0]):
            acc = acc + pf[:, k:k + 1] * pd[k][None]
    v_posed = v_shaped[None] + acc.reshape(F, V, 3)
    GR, Gt = np.zeros((F, J, 3, 3), dt), np.zeros((F, J, 3), dt)
    GR[:, 0], Gt[:, 0] = R[:, 0], J_rest[0]
    for j in range(1, J):
        p = int(parents[j])
        assert 0 <= p < j
        GR[:, j] = _mm3(GR[:, p], R[:, j])
        Gt[:, j] = _mv3(GR[:, p], (J_rest[j] - J_rest[p])[None]) + Gt[:, p]
    At = Gt - _mv3(GR, J_rest[None])
    out = np.zeros((F, V, 3), dt)
    for j in range(J):
        if not weights[:, j].any():
            continue                                                          # (adds exact zeros)
        out = out + weights[None, :, j, None] * (_mv3(GR[:, j, None], v_posed) + At[:, j, None])
    joints = Gt
    if transl is not None:
        t = np.asarray(transl).astype(dt).reshape(F, 1, 3)
        out, joints = out + t, joints + t
    c = np.zeros(3, dt) if centre is None else np.asarray(centre).astype(dt)
    out, joints = (out - c) * dt(scale), (joints - c) * dt(scale)
    assert out.dtype == dt and joints.dtype == dt
    return out, joints


def make_poses(kind, F, J, seed=0):
    """zero: exactly zero; tiny: norm 1e-6; random: uniform directions, angles up to pi; pi: one joint per frame at exactly
    fp32 pi about an axis, the others random"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "zero":
        return np.zeros((F, J, 3), np.float32)
    d = rng.standard_normal((F, J, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    if kind == "tiny":
        return (d * 1e-6).astype(np.float32)
    p = (d * rng.uniform(0.0, np.pi, (F, J, 1))).astype(np.float32)
    if kind == "pi":
        for f in range(F):
            j = (f * 7 + J // 2) % J
            p[f, j] = 0.0
            p[f, j, f % 3] = np.float32(np.pi)
    elif kind != "random":
        raise ValueError(kind)
    return p


def _case(V, J=55, tree="smplx", width=4, pose_blend=True, F=2, poses="random", transl=True, affine=True):
    return dict(V=V, J=J, tree=tree, width=min(width, J), pose_blend=pose_blend and J > 1, F=F, poses=poses, transl=transl,
                affine=affine)


def sweep_cases(verts_per_thread, verts_per_wave, verts_per_workgroup, frame_tile):
    """The boundary sweep: not the full product - every value of every axis at least once against a non-trivial partner."""
    T = frame_tile
    vs = {1, 3, 4, 5, 63, 64, 65, 255, 256, 257}
    for c in (verts_per_thread, verts_per_wave, verts_per_workgroup, 2 * verts_per_workgroup):
        vs |= {c - 1, c, c + 1}
    cases = [_case(V) for V in sorted(v for v in vs if v >= 1)]
    cases += [
        _case(65, J=1, tree="star", width=1, pose_blend=False), _case(5, J=1, tree="chain", width=1, F=T + 1),
        _case(65, J=2, tree="chain", width=1), _case(257, J=2, tree="star", width=2, pose_blend=False, F=1),
        _case(65, J=55, tree="chain", width=5), _case(129, J=55, tree="star", width=55, F=1),
        _case(257, J=55, tree="smplx", width=4, pose_blend=False, F=T),
        _case(65, J=64, tree="chain", width=64, F=T + 1), _case(257, J=64, tree="star", width=4, F=1),
        _case(129, J=64, tree="smplx", width=5, pose_blend=False), _case(63, J=64, tree="chain", width=1, F=1, poses="pi"),
    ]
    cases += [_case(257, F=F) for F in (1, T, T + 1, 136)]                # (F = 2 at V = 257 is part of the V sweep)
    cases += [_case(65, F=F, poses=kind) for kind in ("zero", "tiny", "random", "pi") for F in (1, T + 1)]
    cases += [_case(129, J=64, tree="chain", width=5, F=2, poses=kind) for kind in ("zero", "tiny", "pi")]
    cases += [_case(65, transl=False, affine=False), _case(65, transl=True, affine=False), _case(65, transl=False, affine=True),
              _case(257, J=64, tree="smplx", width=64, F=T + 1, transl=False, affine=True)]
    for i, c in enumerate(cases):
        c["seed"] = i
        c["id"] = "V{V}-J{J}{tree}-w{width}-K{k}-F{F}-{poses}-t{t}a{a}".format(k=9 * (c["J"] - 1) if c["pose_blend"] else 0,
                                                                               t=int(c["transl"]), a=int(c["affine"]), **c)
    return cases


_BUILT = {}


def build_case(case):
    """body, inputs and both restatements of a case: computed once per process and left unchanged"""
    key = case["id"]
    if key in _BUILT:
        return _BUILT[key]
    body = make_body(case["V"], case["J"], case["tree"], case["width"], case["pose_blend"], seed=case["seed"])
    rng = np.random.default_rng(5000 + case["seed"])
    betas = rng.standard_normal(3)
    poses = make_poses(case["poses"], case["F"], case["J"], seed=case["seed"])
    transl = rng.uniform(-0.5, 0.5, (case["F"], 3)).astype(np.float32) if case["transl"] else None
    centre = rng.uniform(-0.3, 0.3, 3).astype(np.float32) if case["affine"] else None
    scale = float(np.float32(1.7)) if case["affine"] else 1.0
    v_shaped, J_rest = setup(body, betas)
    args = (v_shaped.astype(np.float32), J_rest.astype(np.float32), body["parents"], body["weights"], body["posedirs"], poses)
    kw = dict(transl=transl, centre=centre, scale=scale)
    v64, j64 = pose(*args, dtype=np.float64, **kw)
    v32, j32 = pose(*args, dtype=np.float32, **kw)
    vmax = max(float(np.abs(v64).max()), float(np.abs(j64).max()))
    ref_err = max(float(np.abs(v32 - v64).max()), float(np.abs(j32 - j64).max()))
    out = dict(body=body, betas=betas, poses=poses, transl=transl, centre=centre, scale=scale, v64=v64, j64=j64, vmax=vmax,
               ref_err=ref_err)
    _BUILT[key] = out
    return out
