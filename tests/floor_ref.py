"""Float64 numpy restatement of mmego_floor_stats and mmego_floor_clamp, written from the recipe (include/mmego_hip.h), row by row and
leg by leg with plain vectors -- not from the kernel.  Also the random legs the CPU and GPU tests draw."""
import numpy as np

FLOOR_W = 22
FEET = ((3, 15, 0), (7, 19, 1))          # (local joint of the lower row, joint of the 21-joint target, contact column)
LEGS = ((0, 1, 2, 3), (4, 5, 6, 7))      # (hip, knee, ankle, foot) in local joints


def plane(g):
    """-> (n / |n|, d / |n|) of one plane (a, b, c, d), or None where |n| is not > 1e-6."""
    g = np.asarray(g, dtype=np.float64)
    n = np.linalg.norm(g[:3])
    if not n > 1e-6:
        return None
    return g[:3] / n, g[3] / n


def height(pl, x):
    return float(np.dot(pl[0], x) + pl[1])


def stats(lo, tgt, ground, contact, seg, H):
    """-> (out [rows, 22] float64, hp [rows, 2], ht [rows, 2]); the heights NaN on the rows that write zeros."""
    lo = np.asarray(lo, dtype=np.float64).reshape(len(lo), 8, 3)
    tgt = np.asarray(tgt, dtype=np.float64).reshape(len(lo), 21, 3)
    out = np.zeros((len(lo), FLOOR_W))
    hp, ht = np.full((len(lo), 2), np.nan), np.full((len(lo), 2), np.nan)
    for r in range(len(lo)):
        pl = plane(ground[r])
        if seg[r] < 0 or pl is None:
            continue
        for k, (jl, jt, col) in enumerate(FEET):
            p, t, c = height(pl, lo[r, jl]), height(pl, tgt[r, jt]), float(contact[r, col])
            hp[r, k], ht[r, k] = p, t
            out[r, 11 * k:11 * k + 11] = [abs(p - t), max(0.0, -p), p < 0, p < H, (p < H) * c, c, c * max(0.0, p),
                                          max(0.0, -t), t < 0, t < H, (t < H) * c]
    return out, hp, ht


def _without(x, u):
    return x - np.dot(x, u) * u


def leg(Hp, K, A, T, pl, margin):
    """One leg in float64.  -> dict: K, A, T (the new joints), lift (what the leg was raised by, 0 where it stays), fallback (0 / 1),
    b (the knee's distance from the hip-ankle line, None where the leg stays), edge (how close D came to a reach limit, inf where the
    leg stays: where it is tiny, float32 may fall on the other side)."""
    n, d = pl
    stay = dict(K=K, A=A, T=T, lift=0.0, fallback=0, b=None, edge=np.inf)
    lift = max(0.0, margin - height(pl, T), margin - height(pl, A))
    if not lift > 0.0:
        return stay
    l1, l2 = np.linalg.norm(K - Hp), np.linalg.norm(A - K)
    v = A + lift * n - Hp
    D = np.linalg.norm(v)
    if not D > 1e-9:
        return dict(stay, fallback=1)
    u = v / D
    near, far = abs(l1 - l2) + 1e-6 * (l1 + l2), (l1 + l2) * (1.0 - 1e-6)
    Dc = min(max(D, near), far)
    a = (l1 * l1 - l2 * l2 + Dc * Dc) / (2.0 * Dc)
    b = np.sqrt(max(0.0, l1 * l1 - a * a))
    w = _without(K - Hp, u)
    if np.linalg.norm(w) < 1e-4 * l1 or np.linalg.norm(w) == 0.0:
        w = _without(T - A, u)
        if np.linalg.norm(w) < 1e-4 * np.linalg.norm(T - A) or np.linalg.norm(w) == 0.0:
            w = _without(np.eye(3)[int(np.argmin(np.abs(u)))], u)          # (argmin: the first on ties)
    w = w / np.linalg.norm(w)
    K2, A2 = Hp + a * u + b * w, Hp + Dc * u
    T2 = A2 + (T - A)
    if not np.isfinite(np.concatenate([K2, A2, T2])).all():
        return dict(stay, fallback=1)
    return dict(K=K2, A=A2, T=T2, lift=lift, fallback=int(Dc != D), b=b, edge=min(abs(D - near), abs(D - far)))


def clamp(src, ground, seg, margin):
    """-> (dst [rows, 24] float64, lifted [rows], fallback [rows], legs): legs[r][l] the dict of leg() (None on rows that are copied)."""
    x = np.asarray(src, dtype=np.float64).reshape(len(src), 8, 3)
    dst, lifted, fallback, legs = x.copy(), np.zeros(len(x)), np.zeros(len(x), dtype=np.int32), []
    for r in range(len(x)):
        pl = plane(ground[r])
        if seg[r] < 0 or pl is None:
            fallback[r] = 2 if seg[r] >= 0 else 0
            legs.append((None, None))
            continue
        both = []
        for h, k, a, t in LEGS:
            res = leg(x[r, h], x[r, k], x[r, a], x[r, t], pl, margin)
            dst[r, k], dst[r, a], dst[r, t] = res["K"], res["A"], res["T"]
            lifted[r], fallback[r] = max(lifted[r], res["lift"]), fallback[r] + res["fallback"]
            both.append(res)
        legs.append(tuple(both))
    return dst.reshape(len(x), 24), lifted, fallback, legs


def random_legs(rng, n):
    """n rows of two random standing legs with their planes: a hip near z = 0.95, a thigh of about 0.42 m to a knee 15 cm forward, a
    shank of about 0.38 m back to an ankle near z = 0.20, a foot bone forward and down to z near 0.04, sideways offsets of sigma 3 to 8 cm
    on knee and ankle, a plane normal within 2 % of z and d ~ N(-0.02, 0.04): about a third of the legs reach under the plane, and the
    bent knee keeps most of them away from the straight leg, where the knee's side is badly conditioned.
    -> (rows [n, 24] float64, ground [n, 4] float64)."""
    rows = np.zeros((n, 8, 3))
    for l, side in enumerate((-0.1, 0.1)):
        hip = np.stack([rng.normal(0.0, 0.05, n), side + rng.normal(0.0, 0.02, n), 0.95 + rng.normal(0.0, 0.03, n)], axis=1)
        sig = rng.uniform(0.03, 0.08, (n, 1))
        knee = hip + np.array([0.15, 0.0, -0.392]) + np.concatenate([rng.normal(0.0, 1.0, (n, 2)) * sig, rng.normal(0.0, 0.01, (n, 1))], axis=1)
        ankle = knee + np.array([-0.13, 0.0, -0.357]) + np.concatenate([rng.normal(0.0, 1.0, (n, 2)) * sig, rng.normal(0.0, 0.01, (n, 1))], axis=1)
        foot = ankle + np.array([0.12, 0.0, -0.16]) + rng.normal(0.0, 0.02, (n, 3))
        rows[:, 4 * l], rows[:, 4 * l + 1], rows[:, 4 * l + 2], rows[:, 4 * l + 3] = hip, knee, ankle, foot
    normal = np.concatenate([rng.normal(0.0, 0.01, (n, 2)), np.ones((n, 1))], axis=1)
    ground = np.concatenate([normal, rng.normal(-0.02, 0.04, (n, 1))], axis=1)
    return rows.reshape(n, 24), ground
