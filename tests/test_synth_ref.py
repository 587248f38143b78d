"""The fp64 restatement of the device panel generator (tests/synth_ref.py) against the model it states, on the CPU.

tests/test_gpu_synth_pack.py compares synth_kernel with synth_ref cell by cell, and synth_ref shares the kernel's RNG design
(counter keys, one hash, two 24-bit uniforms, Box-Muller).  A weakness of that design would pass the comparison, so the
design is checked here on its own: the latent values must be what gauss_amd/synth.py's model says -- standard normal at
every SNP, AR(1) along the SNPs with the given rho, independent between the two haplotypes and between samples -- and
the genotypes must have the model's frequencies.  Every bound is 5 standard errors of the statistic under the model
(one check in 1.7 million fails by chance; the seeds are committed, so a pass is a pass for good)."""
import numpy as np
import pytest

import synth_ref

N, S, SEED = 20_000, 40, 20260213
K = 5.0                             # standard errors allowed


@pytest.fixture(scope="module")
def lat():
    rng = np.random.default_rng(1)
    rho = rng.uniform(0.5, 0.999, size=S).astype(np.float32)
    rho[0] = 1.0
    z0, z1 = synth_ref.latents(S, N, rho, SEED)
    return dict(rho=rho.astype(np.float64), z0=z0, z1=z1, both=np.concatenate([z0, z1], axis=1))


def _corr(a, b):
    a = a - a.mean(axis=1, keepdims=True)
    b = b - b.mean(axis=1, keepdims=True)
    return (a * b).sum(axis=1) / np.sqrt((a * a).sum(axis=1) * (b * b).sum(axis=1))


def test_mix64_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 (state = 0, gamma added before mixing) -- published test vector
    state, want = 0, [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for w in want:
        assert int(synth_ref.mix64(np.array([state], dtype=np.uint64))[0]) == w
        state = (state + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)


def test_latent_values_are_standard_normal_at_every_snp(lat):
    z = lat["both"]
    n = z.shape[1]
    assert np.max(np.abs(z.mean(axis=1))) <= K / np.sqrt(n)                       # se of a mean of n N(0,1) values
    assert np.max(np.abs((z * z).mean(axis=1) - 1.0)) <= K * np.sqrt(2.0 / n)     # var(z^2) = 2
    # the tails carry the thresholds of rare alleles: P(z < -2) and P(z > 2), binomial
    from scipy.stats import norm
    p = norm.cdf(-2.0)
    se = np.sqrt(p * (1 - p) / n)
    assert np.max(np.abs((z < -2.0).mean(axis=1) - p)) <= K * se
    assert np.max(np.abs((z > 2.0).mean(axis=1) - p)) <= K * se


def test_lag_one_correlation_is_rho(lat):
    z = lat["both"]
    r = _corr(z[1:], z[:-1])
    # Fisher: atanh(r) ~ N(atanh(rho), 1 / (n - 3)), accurate up to rho = 0.999
    assert np.max(np.abs(np.arctanh(r) - np.arctanh(lat["rho"][1:]))) <= K / np.sqrt(z.shape[1] - 3)


def test_the_two_haplotypes_are_uncorrelated(lat):
    assert np.max(np.abs(_corr(lat["z0"], lat["z1"]))) <= K / np.sqrt(N)


def test_adjacent_samples_are_uncorrelated(lat):
    for z in (lat["z0"], lat["z1"]):
        assert np.max(np.abs(_corr(z[:, 1:], z[:, :-1]))) <= K / np.sqrt(N - 1)
    assert np.max(np.abs(_corr(lat["z0"][:, 1:], lat["z1"][:, :-1]))) <= K / np.sqrt(N - 1)


def test_every_cell_has_a_key_of_its_own():
    keys = [synth_ref.first_keys(SEED, N)] + [synth_ref.innovation_keys(SEED, s, N) for s in range(1, S)]
    assert len(np.unique(np.concatenate(keys))) == S * N
    # a seed with high bits: seed ^ (s << 32) is no longer seed + (s << 32)
    big = synth_ref.exact_inputs()["seed"]
    keys = [synth_ref.first_keys(big, N)] + [synth_ref.innovation_keys(big, s, N) for s in range(1, S)]
    assert len(np.unique(np.concatenate(keys))) == S * N


def test_rho_one_repeats_the_snp_and_rho_zero_forgets_it():
    rho = np.array([1.0, 0.7, 1.0, 0.0, 0.9], dtype=np.float32)
    z0, z1 = synth_ref.latents(5, 4096, rho, 99)
    assert np.array_equal(z0[2], z0[1]) and np.array_equal(z1[2], z1[1])
    e0, e1 = synth_ref.normal2(synth_ref.innovation_keys(99, 3, 4096))
    assert np.array_equal(z0[3], e0) and np.array_equal(z1[3], e1)


def test_genotypes_have_the_frequencies_of_the_threshold_model():
    """gauss_amd/synth.py: allele = latent < thr, thr = Phi^-1(p): per population the allele frequency is p and the
    heterozygote share 2p(1-p)."""
    from scipy.stats import norm
    rng = np.random.default_rng(2)
    off = synth_ref.pop_offsets([7000, 6001, 6999])
    rho = rng.uniform(0.5, 0.999, size=S).astype(np.float32)
    thr = norm.ppf(rng.uniform(0.02, 0.98, size=(S, 3))).astype(np.float32)
    G, z0, z1, t = synth_ref.synth(S, off, thr, rho, SEED)
    assert G.dtype == np.uint8 and G.shape == (S, N) and G.max() <= 2
    assert np.array_equal(t[:, 6999], thr[:, 0].astype(np.float64)) and np.array_equal(t[:, 7000], thr[:, 1].astype(np.float64))
    assert np.array_equal(t[:, 13000], thr[:, 1].astype(np.float64)) and np.array_equal(t[:, 13001], thr[:, 2].astype(np.float64))
    za, zh = synth_ref.frequency_excess(G, off, thr)
    assert np.max(np.abs(za)) <= K, np.max(np.abs(za))
    assert np.max(np.abs(zh)) <= K, np.max(np.abs(zh))


def test_exact_inputs_keep_few_cells_next_to_a_threshold():
    """What the cell-by-cell comparison on the device assumes of its inputs: at most 1 % of the reference's cells have a
    latent value within DELTA of the threshold (the model gives 2 * 2 DELTA * phi(thr) <= 0.16 %)."""
    a = synth_ref.exact_inputs()
    G, z0, z1, t = synth_ref.synth(a["S"], a["off"], a["thr"], a["rho"], a["seed"])
    share = float((synth_ref.margin(z0, z1, t) <= synth_ref.DELTA).mean())
    print(f"share of cells within {synth_ref.DELTA} of a threshold: {share:.5f}")
    assert 0.0 < share <= 0.01
    assert np.array_equal(z0[17], z0[16]) and np.array_equal(z1[17], z1[16])      # rho[17] = 1


def test_reference_meets_the_frequencies_in_the_bench_regime():
    a = synth_ref.bench_regime_inputs()
    G, _, _, _ = synth_ref.synth(a["S"], a["off"], a["thr"], a["rho"], a["seed"])
    za, zh = synth_ref.frequency_excess(G, a["off"], a["thr"])
    print(f"largest excess in standard errors: allele frequency {np.max(np.abs(za)):.2f}, heterozygotes {np.max(np.abs(zh)):.2f}")
    assert np.max(np.abs(za)) <= K
    assert np.max(np.abs(zh)) <= K
    r = synth_ref.adjacent_correlation(G, a["off"])
    assert np.all(np.isfinite(r)) and r.min() > 0.0           # no monomorphic SNP; neighbours in positive LD
