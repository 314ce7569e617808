"""The cases of the Fourier-curve solver (TEST infrastructure): what goldens_fourier.json freezes and what the GPU tests run, each at
the smallest shape at which its part of the kernel can go wrong (tests/_fourier_oracle.py states the expected result)."""
import hashlib

import numpy as np

import _fourier_oracle as FO
import _sa_cases as K


def o(k_max=2, m=17, epochs=3, lam=0.05, lambda_decay=0.5, lr=0.05):
    return dict(k_max=k_max, m=m, epochs=epochs, lam=lam, lambda_decay=lambda_decay, lr=lr)


def circle(n):
    """the reference's own unit-test instance (fourier.rs:118-128): f64 cos and sin rounded to f32"""
    i = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.cos(2.0 * np.pi * i / n), np.sin(2.0 * np.pi * i / n)], axis=1).astype(np.float32))


def stacked(n):
    """cities in clusters of identical points: several cities share one sample, the decode's order falls to the city position"""
    a = K.small(4)
    return np.ascontiguousarray(np.concatenate([a] * ((n + 3) // 4))[:n])


# name -> (xy, packed, n, opts)
def cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    a = K.tsplib("a280")
    out = {
        "n2": (K.small(2), None, 2, o()),
        "n3": (K.small(3), None, 3, o()),
        "circle5": (circle(5), None, 5, o(2, 50, 20)),                 # fourier.rs:130-137 fast_opts: symmetric cities, tied roots
        "m2_k1": (K.small(7), None, 7, o(1, 2, 4)),
        "m63": (K.small(9), None, 9, o(2, 63, 3)),
        "m64": (K.small(9), None, 9, o(2, 64, 3)),
        "m65": (K.small(9), None, 9, o(2, 65, 3)),
        "m4096_k32": (K.small(5), None, 5, o(32, 4096, 1)),
        "epochs1": (K.small(9), None, 9, o(3, 20, 1)),
        "stages_k3_e2": (K.small(11), None, 11, o(3, 31, 2)),
        "n65_past_64_lanes": (K.small(65), None, 65, o(2, 30, 2)),     # run with threads = 64: n = threads + 1
        "n63_chunk": (K.small(63), None, 63, o(2, 30, 2)),             # chunk 64: n = chunk - 1, chunk, chunk + 1
        "n64_chunk": (K.small(64), None, 64, o(2, 30, 2)),
        "n129_two_chunks": (K.small(129), None, 129, o(2, 30, 2)),
        "stacked": (stacked(14), None, 14, o(2, 9, 3)),
        "gr17_matrix": (g["xy"], g["packed"], 17, o(3, 40, 5)),
        "berlin52": (b["xy"], None, 52, dict(FO.DEFAULTS)),
        "a280": (a["xy"], None, 280, dict(FO.DEFAULTS, epochs=50)),
    }
    return out


GOLDEN = ("n2", "circle5", "m2_k1", "m65", "epochs1", "stages_k3_e2", "n65_past_64_lanes", "stacked", "gr17_matrix", "berlin52")
LOG_CAP = 64  # steps whose sample indices a test compares (berlin52 runs 1 600)


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=dtype)).astype(np.dtype(dtype).newbyteorder("<")).tobytes()).hexdigest()


def case_record(res):
    """what goldens_fourier.json freezes of a run"""
    return {"tour": [int(v) for v in res["tour"]], "cost_bits": FO.bits(res["cost"]), "coeffs": [str(int(v)) for v in FO.f64_words(res["coeffs"])],
            "log_sha256": sha(res["log"][:LOG_CAP], np.uint32), "stage_sha256": sha(FO.f64_words(res["stage_c"]), np.uint64),
            "sidx": [int(v) for v in res["sidx"]]}


def oracle(name):
    xy, packed, n, opts = cases()[name]
    return FO.solve_cached(name, xy, packed, n, **opts)


def tied_root_pair():
    """two f32 squares that differ but whose correctly rounded roots are equal: (larger square, smaller square, root).  sqrt halves
    the relative spacing, so neighbouring floats in the upper half of a binade share a root"""
    s = np.float32(3.0)
    while True:
        t = np.nextafter(s, np.float32(4.0))
        if np.sqrt(s, dtype=np.float32) == np.sqrt(t, dtype=np.float32):
            return t, s, np.sqrt(s, dtype=np.float32)
        s = t
