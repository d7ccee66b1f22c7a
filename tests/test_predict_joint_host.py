"""Joint conditional / posterior draws without a GPU: the NumPy restatement of the draw stream of mi_gp_sample_cov
(Philox4x64-10 + Box-Muller, include/mi_gp.h) against numpy.random.Philox, the scratch size query, argument validation of
mi_gp_predict_cov / mi_gp_sample_cov before any HIP call, and BO's refusal of Thompson sampling outside opt_method='predict'."""
import ctypes
import types

import numpy as np
import pytest

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
PHILOX_W = (0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B)


def _mulhilo(a, b):
    """(hi, lo) of the 128-bit product of uint64 arrays, from 32-bit halves (no overflow in any partial sum)."""
    a0, a1, b0, b1 = a & M32, a >> np.uint64(32), b & M32, b >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & M32) + (p10 & M32)
    hi = p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))
    return hi, a * b


def philox_words(seed, blocks):
    """The four words of Philox block b (for each b in `blocks`): Philox4x64-10 of the 256-bit counter b + 1 under the key
    (seed, 0) -- (len(blocks), 4) uint64."""
    b = np.asarray(blocks, dtype=object)
    c0 = np.array([(int(v) + 1) % 2 ** 64 for v in b], dtype=np.uint64)
    c1 = np.array([(int(v) + 1) // 2 ** 64 for v in b], dtype=np.uint64)
    c = [c0, c1, np.zeros_like(c0), np.zeros_like(c0)]
    k0, k1 = int(seed) % 2 ** 64, 0
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(PHILOX_M[0], c[0])
            hi1, lo1 = _mulhilo(PHILOX_M[1], c[2])
            c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
            k0, k1 = (k0 + PHILOX_W[0]) % 2 ** 64, (k1 + PHILOX_W[1]) % 2 ** 64
    return np.stack(c, axis=1)


def philox_normals(seed, offset, count):
    """Normals 0 .. count - 1 of the stream of mi_gp_sample_cov at (seed, offset): normal j from block offset + j // 4,
    words (w0, w1) -> normals 4b, 4b + 1 and (w2, w3) -> 4b + 2, 4b + 3, u = ((w >> 11) + 0.5) 2^-53,
    (rho cos 2 pi u1, rho sin 2 pi u1) with rho = sqrt(-2 log u0)."""
    nb = (count + 3) // 4
    w = philox_words(seed, [int(offset) + q for q in range(nb)])
    u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    out = np.empty((nb, 4))
    for p in range(2):
        rho = np.sqrt(-2.0 * np.log(u[:, 2 * p]))
        out[:, 2 * p] = rho * np.cos(2.0 * np.pi * u[:, 2 * p + 1])
        out[:, 2 * p + 1] = rho * np.sin(2.0 * np.pi * u[:, 2 * p + 1])
    return out.ravel()[:count]


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 63 + 17, 2 ** 64 - 1])
@pytest.mark.parametrize("counter", [0, 1, 7, 2 ** 32 - 1, 2 ** 40 + 3, 2 ** 64 - 1])
def test_philox_restatement_matches_numpy(seed, counter):
    ref = np.random.Philox(key=seed, counter=counter).random_raw(4)
    got = philox_words(seed, [counter])[0]
    assert np.array_equal(got, ref), (got, ref)


def test_philox_restatement_matches_numpy_over_consecutive_blocks():
    bg = np.random.Philox(key=987654321, counter=41)
    ref = bg.random_raw(4 * 50).reshape(50, 4)  # consecutive blocks: counters 42, 43, ...
    assert np.array_equal(philox_words(987654321, range(41, 91)), ref)


def test_box_muller_stream_layout_and_offsets():
    z = philox_normals(5, 0, 4001)
    assert z.shape == (4001,) and np.isfinite(z).all()
    assert abs(z.mean()) < 0.1 and abs(z.std() - 1.0) < 0.05
    # a later offset continues the same stream: block q of offset 10 is block 10 + q of offset 0
    assert np.array_equal(philox_normals(5, 10, 40), z[40:80])
    # a partial last block: the first normals of a block do not depend on how many are taken
    assert np.array_equal(philox_normals(5, 3, 6), philox_normals(5, 3, 8)[:6])


def _lib():
    from andvaranaut_amd import _lib

    return _lib.load()


def test_sample_cov_work_sizes():
    lib = _lib()
    assert lib.mi_gp_sample_cov_work(1, 1) == 8 + 16384 + 2 * 128 * 128
    assert lib.mi_gp_sample_cov_work(300, 20) == 8 + 3 * 16384 + 2 * 128 * 384
    assert lib.mi_gp_sample_cov_work(129, 129) == 8 + 2 * 16384 + 2 * 256 * 256
    assert lib.mi_gp_sample_cov_work(10000, 1) == 8 + 79 * 16384 + 2 * 128 * 10112
    assert lib.mi_gp_sample_cov_work(0, 1) == -1 and lib.mi_gp_sample_cov_work(5, 0) == -1


FAKE = 0x1000  # a non-null address: validation returns before anything is dereferenced


def _sample(lib, h=None, ldc=128, m=10, s=2, ldd=10, work_len=None, ej=0.0, bufs=True):
    p = FAKE if bufs else None
    if work_len is None:
        work_len = max(lib.mi_gp_sample_cov_work(max(m, 1), max(s, 1)), 0)
    return lib.mi_gp_sample_cov(h, p, ldc, m, p, ej, s, 1, 0, p, ldd, p, work_len)


@pytest.mark.parametrize("kw,text", [
    ({}, b"null handle"),
    ({"m": 0}, b"m must be"),
    ({"m": -3}, b"m must be"),
    ({"s": 0}, b"s must be"),
    ({"ldc": 127}, b"ldc"),
    ({"ldc": 129}, b"ldc"),
    ({"m": 129, "ldc": 128, "ldd": 129}, b"ldc"),
    ({"ldd": 9}, b"ldd"),
    ({"work_len": 100}, b"work_len"),
    ({"ej": -1.0}, b"extra_jitter"),
    ({"ej": float("nan")}, b"extra_jitter"),
    ({"bufs": False}, b"null buffer"),
])
def test_sample_cov_rejects_bad_arguments_without_a_gpu(kw, text):
    lib = _lib()
    assert _sample(lib, **kw) == -1
    msg = lib.mi_gp_last_global_error()
    assert b"mi_gp_sample_cov" in msg and text in msg, msg


@pytest.mark.parametrize("m,ldc,bufs,text", [
    (10, 128, True, b"null handle"),
    (0, 128, True, b"m must be"),
    (10, 127, True, b"ldc"),
    (10, 126, True, b"ldc"),
    (200, 255, True, b"ldc"),
    (10, 128, False, b"null buffer"),
])
def test_predict_cov_rejects_bad_arguments_without_a_gpu(m, ldc, bufs, text):
    lib = _lib()
    p = FAKE if bufs else None
    assert lib.mi_gp_predict_cov(None, p, m, p, 1024, p, p, ldc, 1) == -1
    msg = lib.mi_gp_last_global_error()
    assert b"mi_gp_predict_cov" in msg and text in msg, msg


@pytest.mark.parametrize("opt_method", ["DE", "map", "mcmc_mean", "mcmc_map"])
def test_bo_rejects_thompson_sampling_outside_predict(opt_method):
    from andvaranaut_amd.consumers import ConsumersMixin

    with pytest.raises(ValueError, match="TS"):
        ConsumersMixin.BO(types.SimpleNamespace(), method="TS", opt_method=opt_method)
