"""hgibbs_beta_sqnorm against a plain sequential sum per group in marker order, bit for bit (src/BayesRRm.cpp:2496-2499
adds beta^2 marker by marker; the device only compacts the non-zero effects, the adds and their order stay)."""
import numpy as np
import pytest

from hydra_amd import capi, synth

pytestmark = pytest.mark.gpu

N = 64


def device(M, G):
    geno = synth.make_genotypes(M, N, seed=5, missing_rate=0.0)
    dev = capi.Device(0)
    dev.load_bed(synth.pack_bed_columns(geno), N)
    groups = (np.arange(M) % G).astype(np.int32)
    cva = np.tile(np.array([0.0, 0.01, 0.1]), (G, 1))
    cvai = np.where(cva > 0, 1.0 / np.where(cva > 0, cva, 1.0), 0.0)
    dev.set_model(groups, cva, cvai)
    return dev, groups


def sequential(beta, groups, G):
    out = [np.float64(0.0)] * G
    for b, g in zip(beta.tolist(), groups.tolist()):
        out[g] = np.float64(out[g] + np.float64(b) * np.float64(b))
    return np.array(out, dtype=np.float64)


def planted(M, share, seed):
    rng = np.random.default_rng(seed)
    beta = np.zeros(M)
    k = int(round(share * M))
    at = rng.choice(M, size=k, replace=False)
    beta[at] = rng.standard_normal(k) * 10.0 ** rng.integers(-6, 3, size=k)
    return beta


CASES = [
    ("all zero", 20000, 1, lambda M: np.zeros(M)),
    ("1 % non-zero, one group", 20000, 1, lambda M: planted(M, 0.01, 1)),
    ("1 % non-zero, three groups", 20000, 3, lambda M: planted(M, 0.01, 2)),
    ("negative zeros", 20000, 3, lambda M: np.where(np.arange(M) % 7 == 0, -0.0, planted(M, 0.01, 3))),
    ("only negative zeros", 5000, 1, lambda M: np.full(M, -0.0)),
    ("dense: the whole vector is fetched", 20000, 3, lambda M: planted(M, 1.0, 4)),
    ("just above half", 20000, 3, lambda M: planted(M, 0.51, 5)),
    ("just below half", 20000, 3, lambda M: planted(M, 0.49, 6)),
    ("M not a multiple of the chunk", 4096 * 3 + 17, 3, lambda M: planted(M, 0.01, 7)),
    ("M below one chunk", 37, 1, lambda M: planted(M, 0.3, 8)),
    ("more entries than the first fetch guesses", 300000, 3, lambda M: planted(M, 0.05, 9)),
]


@pytest.mark.parametrize("name,M,G,make", CASES, ids=[c[0] for c in CASES])
def test_beta_sqnorm_is_the_sequential_sum(gpu_lib, name, M, G, make):
    dev, groups = device(M, G)
    beta = np.ascontiguousarray(make(M), dtype=np.float64)
    dev.set_beta(beta)
    want = sequential(beta, groups, G)
    for call in range(2):  # the second call starts from the first one's guess of the list's length
        got = dev.beta_sqnorm()
        assert got.dtype == np.float64 and got.shape == (G,)
        assert got.tobytes() == want.tobytes(), "%s, call %d: %r != %r" % (name, call, got, want)
    back, _, _ = dev.get_beta()
    assert back.tobytes() == beta.tobytes()  # the effects themselves are not touched


def test_sparse_after_dense_and_back(gpu_lib):
    M, G = 50000, 3
    dev, groups = device(M, G)
    for share, seed in ((1.0, 11), (0.01, 12), (0.6, 13), (0.0, 14), (0.02, 15)):
        beta = planted(M, share, seed)
        dev.set_beta(beta)
        assert dev.beta_sqnorm().tobytes() == sequential(beta, groups, G).tobytes()
