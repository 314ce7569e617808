"""The Fourier-curve solver's specification (teeline_amd/csrc/fourier_spec.h) stated in numpy and, for the small
cases, in literal Python loops (TEST infrastructure).  fourier.rs:10-312's sequence of operations with the five departures of the
specification; `arith="libm"` takes the reference's own arithmetic for departures 1 and 2 instead (libm cos and sin of the rounded
angle 2 pi k (j / m), hypot) — used ONLY to measure the departures: the reference itself was never run, and its kd-tree's choice
among tied samples cannot be restated (departure 3 stands in both variants)."""
import math

import numpy as np

from _sa_oracle import dist_fn, tour_length
from _som_oracle import cossin2pi
from _swarm_oracle import cached

DEFAULTS = dict(k_max=4, m=200, lam=0.05, lambda_decay=0.5, lr=0.05, epochs=400)  # mod.rs:1341-1352
TWO_PI = 6.283185307179586
MAX_K, MAX_M, MAX_N = 32, 4096, 65536
# fourier_spec.h's measured constants (test_fourier_oracle.py measures them again)
BASIS_MEASURED_ABS_DIFF = 3.6e-14
MEASURED = {"berlin52": dict(moved=0, ties=1), "a280": dict(moved=0, ties=0)}  # default options, spec against the libm variant


def validate(k_max, m, lam, lambda_decay, lr, epochs):  # mod.rs:1354-1384
    if k_max < 1:
        raise ValueError("k_max must be >= 1")
    if m < 2:
        raise ValueError("m must be >= 2")
    if not lam > 0.0:
        raise ValueError("lambda must be > 0")
    if not 0.0 < lambda_decay < 1.0:
        raise ValueError("lambda_decay must be in (0, 1)")
    if not lr > 0.0:
        raise ValueError("lr must be > 0")
    if epochs < 1:
        raise ValueError("epochs must be >= 1")


def basis_table(m):
    """E[r] = (cos, sin)(2 pi r / m) by som_spec.h's exact reduction: [m, 2]"""
    c, s = cossin2pi(np.arange(m, dtype=np.float64) / np.float64(m))
    return np.stack([c, s], axis=1)


def index_matrix(k_max, m):
    """R[ki, j] = (k j) mod m, the non-negative remainder"""
    k = np.arange(-k_max, k_max + 1, dtype=np.int64)
    return (k[:, None] * np.arange(m, dtype=np.int64)[None, :]) % m


def basis_spec(k_max, m):
    """B[ki, j] = E[(k j) mod m]: (re [L, m], im [L, m])"""
    E, R = basis_table(m), index_matrix(k_max, m)
    return E[R, 0], E[R, 1]


def basis_libm(k_max, m):
    """fourier.rs:263-273: exp(i 2 pi k s), s = j / m, the angle rounded as the reference rounds it"""
    k = np.arange(-k_max, k_max + 1, dtype=np.float64)
    s = np.arange(m, dtype=np.float64) / np.float64(m)
    th = ((2.0 * math.pi) * k[:, None]) * s[None, :]
    return np.cos(th), np.sin(th)


def init_coefficients(xy, k_max, arith="spec"):
    """fourier.rs:23-32, 53-58: sequential sums in city order"""
    z = np.asarray(xy, dtype=np.float32).astype(np.float64)
    n = len(z)
    zero = np.zeros(1)
    cr = np.add.accumulate(np.concatenate([zero, z[:, 0]]))[-1] / np.float64(n)
    ci = np.add.accumulate(np.concatenate([zero, z[:, 1]]))[-1] / np.float64(n)
    dr, di = z[:, 0] - cr, z[:, 1] - ci
    mod = np.hypot(dr, di) if arith == "libm" else np.sqrt((dr * dr) + (di * di))
    radius = np.add.accumulate(np.concatenate([zero, mod]))[-1] / np.float64(n)
    c = np.zeros((2 * k_max + 1, 2))
    c[k_max] = (cr, ci)
    c[k_max + 1] = (radius * 0.5, 0.0)
    return c


def gamma_of(c, Br, Bi):
    """eval_curve: from zero, the modes in order; num_complex's product"""
    gr, gi = np.zeros(Br.shape[1]), np.zeros(Br.shape[1])
    for ki in range(len(c)):
        pr = (c[ki, 0] * Br[ki]) - (c[ki, 1] * Bi[ki])
        pi = (c[ki, 0] * Bi[ki]) + (c[ki, 1] * Br[ki])
        gr, gi = gr + pr, gi + pi
    return gr, gi


def roots(gr, gi, xy32):
    """[n, m] f32: sqrt(dx dx + dy dy), dx = sample - city, every operation rounded to f32"""
    sx, sy = gr.astype(np.float32), gi.astype(np.float32)
    with np.errstate(all="ignore"):
        dx, dy = sx[None, :] - xy32[:, 0][:, None], sy[None, :] - xy32[:, 1][:, None]
        return np.sqrt((dx * dx) + (dy * dy), dtype=np.float32)


def nearest(gr, gi, xy32, count_ties=False):
    """departure 3: the least (key, j); key = the root's bits, 0xFFFFFFFF for a NaN"""
    d = roots(gr, gi, xy32)
    key = np.where(np.isnan(d), np.uint32(0xFFFFFFFF), d.view(np.uint32)).astype(np.uint64)
    packed = (key << np.uint64(32)) | np.arange(d.shape[1], dtype=np.uint64)[None, :]
    idx = (packed.min(axis=1) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if count_ties:
        return idx, int(((key == key.min(axis=1)[:, None]).sum(axis=1) >= 2).sum())
    return idx


def step_numpy(c, Br, Bi, z, xy32, k_max, k_active, lam, lr_over_n, count_ties=False):
    """gradient_step (fourier.rs:276-312): (new c, sample indices, tied queries)"""
    gr, gi = gamma_of(c, Br, Bi)
    res = nearest(gr, gi, xy32, count_ties)
    idx, ties = res if count_ties else (res, 0)
    er, ei = gr[idx] - z[:, 0], gi[idx] - z[:, 1]                      # [n]
    br, bi = Br[:, idx].T, -Bi[:, idx].T                              # conj: [n, L]
    tr = (er[:, None] * br) - (ei[:, None] * bi)
    ti = (er[:, None] * bi) + (ei[:, None] * br)
    zero = np.zeros((1, tr.shape[1]))
    with np.errstate(all="ignore"):
        gradr = np.add.accumulate(np.concatenate([zero, tr]), axis=0)[-1]  # sequential, city order, from zero
        gradi = np.add.accumulate(np.concatenate([zero, ti]), axis=0)[-1]
        k = np.arange(-k_max, k_max + 1)
        t = TWO_PI * k.astype(np.float64)
        w = lam * (t * t)
        gradr, gradi = gradr + (w * c[:, 0]), gradi + (w * c[:, 1])
        new = c.copy()
        act = np.abs(k) <= k_active
        new[act, 0] = c[act, 0] - (lr_over_n * gradr[act])
        new[act, 1] = c[act, 1] - (lr_over_n * gradi[act])
    return new, idx, ties


def step_literal(c, E, z, xy32, k_max, m, k_active, lam, lr_over_n):
    """the same step in plain loops over Python floats (f64, never fused) and np.float32 scalars"""
    L = 2 * k_max + 1
    gam = []
    for j in range(m):
        gr = gi = 0.0
        for ki in range(L):
            r = ((ki - k_max) * j) % m
            ar, ai, br, bi = float(c[ki, 0]), float(c[ki, 1]), float(E[r, 0]), float(E[r, 1])
            gr, gi = gr + ((ar * br) - (ai * bi)), gi + ((ar * bi) + (ai * br))
        gam.append((gr, gi))
    idx = []
    with np.errstate(all="ignore"):
        for ci in range(len(z)):
            best = None
            for j in range(m):
                dx, dy = np.float32(gam[j][0]) - xy32[ci, 0], np.float32(gam[j][1]) - xy32[ci, 1]
                d = np.sqrt(np.float32(dx * dx) + np.float32(dy * dy), dtype=np.float32)
                key = 0xFFFFFFFF if np.isnan(d) else int(np.float32(d).view(np.uint32))
                if best is None or (key, j) < best:
                    best = (key, j)
            idx.append(best[1])
    grad = [[0.0, 0.0] for _ in range(L)]
    for ci in range(len(z)):
        j = idx[ci]
        er, ei = gam[j][0] - float(z[ci, 0]), gam[j][1] - float(z[ci, 1])
        for ki in range(L):
            r = ((ki - k_max) * j) % m
            br, bi = float(E[r, 0]), -float(E[r, 1])
            grad[ki][0] = grad[ki][0] + ((er * br) - (ei * bi))
            grad[ki][1] = grad[ki][1] + ((er * bi) + (ei * br))
    new = c.copy()
    for ki in range(L):
        k = ki - k_max
        t = TWO_PI * float(k)
        w = lam * (t * t)
        for q in range(2):
            g = grad[ki][q] + (w * float(c[ki, q]))
            if abs(k) <= k_active:
                new[ki, q] = float(c[ki, q]) - (lr_over_n * g)
    return new, np.array(idx, dtype=np.int64), 0


def decode(c, Br, Bi, xy32):
    """decode_tour: one more curve, every city's nearest sample, a STABLE sort of the positions by sample"""
    gr, gi = gamma_of(c, Br, Bi)
    idx = nearest(gr, gi, xy32)
    return np.argsort(idx, kind="stable"), idx


def solve(xy, packed, n, *, k_max=4, m=200, lam=0.05, lambda_decay=0.5, lr=0.05, epochs=400, literal=False, arith="spec", log_cap=None, count_ties=False):
    """-> dict(tour positions, cost f32, coeffs [L, 2], log [steps kept, n], stage_c [k_max, L, 2], final sample indices, ties)"""
    validate(k_max, m, lam, lambda_decay, lr, epochs)
    d = dist_fn(xy, packed, n)
    if n < 2:
        return dict(tour=np.arange(n, dtype=np.int64), cost=np.float32(0.0), coeffs=np.zeros((2 * k_max + 1, 2)), log=np.zeros((0, n), dtype=np.int64),
                    stage_c=np.zeros((0, 2 * k_max + 1, 2)), sidx=np.zeros(n, dtype=np.int64), ties=0)
    xy32 = np.ascontiguousarray(np.asarray(xy, dtype=np.float32))
    z = xy32.astype(np.float64)
    c = init_coefficients(xy32, k_max, arith)
    Br, Bi = basis_libm(k_max, m) if arith == "libm" else basis_spec(k_max, m)
    E = basis_table(m)
    lr_over_n = np.float64(lr) / np.float64(n)
    lam_s = np.float64(lam)
    log, stage_c, ties, t = [], [], 0, 0
    for k_active in range(1, k_max + 1):
        for _ in range(epochs):
            if literal:
                c, idx, tq = step_literal(c, E, z, xy32, k_max, m, k_active, float(lam_s), float(lr_over_n))
            else:
                c, idx, tq = step_numpy(c, Br, Bi, z, xy32, k_max, k_active, lam_s, lr_over_n, count_ties)
            ties += tq
            if log_cap is None or t < log_cap:
                log.append(idx)
            t += 1
        stage_c.append(c.copy())
        lam_s = lam_s * np.float64(lambda_decay)  # the running product
    order, sidx = decode(c, Br, Bi, xy32)
    if count_ties:
        ties += nearest(*gamma_of(c, Br, Bi), xy32, True)[1]
    return dict(tour=order.astype(np.int64), cost=tour_length(d, order), coeffs=c, log=np.array(log, dtype=np.int64).reshape(len(log), n),
                stage_c=np.array(stage_c), sidx=sidx, ties=ties)


def energy(c, k_max, m, z, lam):
    """compute_energy of the reference's unit test (fourier.rs:237-260)"""
    Br, Bi = basis_spec(k_max, m)
    gr, gi = gamma_of(c, Br, Bi)
    att = sum(float(np.min((gr - zr) ** 2 + (gi - zi) ** 2)) for zr, zi in z)
    k = np.arange(-k_max, k_max + 1, dtype=np.float64)
    return att + float(np.sum(lam * (TWO_PI * k) ** 2 * (c[:, 0] ** 2 + c[:, 1] ** 2)))


def bits(f):
    return int(np.float32(f).view(np.uint32))


def f64_words(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64).ravel()


solve_cached = cached(solve, lambda res: res)  # (the record is shared and left unchanged; nothing of it is made read-only)
