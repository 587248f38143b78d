"""fp64 restatement of synth_kernel (gauss_amd/csrc/k_misc.hip) for the tests: the same counter-hash keys, the same bits of
the hash for the two uniforms, Box-Muller, the AR(1) recurrence and the threshold, with every floating-point step in float64
(the kernel works in float32 with __logf / __sincosf).  rho and thr are taken as the float32 values the kernel receives.
Besides the genotypes it returns the two latent values of every cell: a cell of the kernel's panel may differ from this one
only where a latent value sits next to its threshold, and the tests need that distance."""
import numpy as np

_M64 = (1 << 64) - 1
_FIRST_MUL = 0x100000001B3          # first-SNP key:  seed * _FIRST_MUL + n
_SAMPLE_MUL = 0x9E3779B1            # innovation key: (seed ^ (s << 32)) + n * _SAMPLE_MUL + 7


def mix64(x):
    """splitmix64's finaliser on uint64 with wraparound (mix64 of k_misc.hip)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def first_keys(seed, n_samples):
    """Key of sample n's latent pair at SNP 0."""
    base = (int(seed) * _FIRST_MUL) & _M64
    with np.errstate(over="ignore"):
        return np.uint64(base) + np.arange(n_samples, dtype=np.uint64)


def innovation_keys(seed, s, n_samples):
    """Key of sample n's innovation pair at SNP s >= 1."""
    base = ((int(seed) ^ (int(s) << 32)) + 7) & _M64
    with np.errstate(over="ignore"):
        return np.uint64(base) + np.arange(n_samples, dtype=np.uint64) * np.uint64(_SAMPLE_MUL)


def normal2(keys):
    """Two independent standard normals per key: u0 from bits 40..63 of the hash, u1 from bits 8..31, each (k + 0.5) / 2^24."""
    h = mix64(keys)
    u0 = ((h >> np.uint64(40)).astype(np.float64) + 0.5) / 16777216.0
    u1 = (((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) + 0.5) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u0))
    a = 2.0 * np.pi * u1
    return r * np.cos(a), r * np.sin(a)


def latents(n_snp, n_samples, rho, seed):
    """(z0, z1), each (n_snp, n_samples) float64: the two AR(1) latent haplotypes of every sample along the SNPs."""
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64)
    z0 = np.empty((n_snp, n_samples))
    z1 = np.empty((n_snp, n_samples))
    z0[0], z1[0] = normal2(first_keys(seed, n_samples))
    for s in range(1, n_snp):
        r = rho[s]
        q = np.sqrt(max(0.0, 1.0 - r * r))
        e0, e1 = normal2(innovation_keys(seed, s, n_samples))
        z0[s] = r * z0[s - 1] + q * e0
        z1[s] = r * z1[s - 1] + q * e1
    return z0, z1


def sample_thresholds(pop_off, thr):
    """(n_snp, n_samples) float64: the threshold of every cell, thr[s, population of the sample]."""
    pop_off = np.asarray(pop_off, dtype=np.int64)
    thr = np.asarray(thr, dtype=np.float32).astype(np.float64)
    pop = np.searchsorted(pop_off[1:-1], np.arange(pop_off[-1]), side="right")
    return thr[:, pop]


def synth(n_snp, pop_off, thr, rho, seed):
    """(G, z0, z1, t): genotypes (n_snp, N) uint8 = (z0 < t) + (z1 < t), the latent pair and the threshold of every cell."""
    n = int(np.asarray(pop_off)[-1])
    z0, z1 = latents(n_snp, n, rho, seed)
    t = sample_thresholds(pop_off, np.asarray(thr)[:n_snp])
    G = (z0 < t).astype(np.uint8) + (z1 < t).astype(np.uint8)
    return G, z0, z1, t


def margin(z0, z1, t):
    """Distance of the nearer latent value of every cell to the cell's threshold."""
    return np.minimum(np.abs(z0 - t), np.abs(z1 - t))


# ------------------------------------------------------------------------------------------
# The committed inputs of the device tests (tests/test_gpu_synth_pack.py).  tests/test_synth_ref.py checks on the CPU what
# those tests assume of them: the share of cells next to a threshold, and that the reference itself has the model's
# frequencies.
# ------------------------------------------------------------------------------------------
DELTA = 1e-3                        # a device cell may differ from the reference only within DELTA of a threshold


def pop_offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def exact_inputs():
    """Three populations whose total (1000) is no multiple of the kernel's 256-thread block; rho[0] = 1 (unused), one rho
    exactly 1 (the SNP repeats the previous latent values), one exactly 0 (a fresh draw), the rest in 0.3 .. 0.99."""
    from scipy.stats import norm
    rng = np.random.default_rng(20261018)
    S, off = 48, pop_offsets([300, 257, 443])
    rho = rng.uniform(0.3, 0.99, size=S).astype(np.float32)
    rho[0], rho[17], rho[29] = 1.0, 1.0, 0.0
    thr = norm.ppf(rng.uniform(0.02, 0.98, size=(S, len(off) - 1))).astype(np.float32)
    return dict(S=S, off=off, rho=rho, thr=np.ascontiguousarray(thr), seed=0x9A3C5F1200C0FFEE)


def bench_regime_inputs():
    """The benchmark's regime: neighbouring SNPs in strong LD (rho 0.993 .. 0.9999), two populations of 4000 samples."""
    from scipy.stats import norm
    rng = np.random.default_rng(20261019)
    S, off = 64, pop_offsets([4000, 4000])
    rho = rng.uniform(0.993, 0.9999, size=S).astype(np.float32)
    rho[0] = 1.0
    thr = norm.ppf(rng.uniform(0.05, 0.95, size=(S, 2))).astype(np.float32)
    return dict(S=S, off=off, rho=rho, thr=np.ascontiguousarray(thr), seed=20260213)


def frequency_excess(G, pop_off, thr):
    """For every (SNP, population): (allele frequency - p) and (heterozygote share - 2p(1-p)), each divided by its binomial
    standard error, p = Phi(thr): 2 n_p independent alleles with probability p, n_p samples heterozygous with probability
    2p(1-p) (the two latent haplotypes of a sample are independent).  Returns two (n_snp, n_pop) arrays."""
    from scipy.stats import norm
    pop_off = np.asarray(pop_off, dtype=np.int64)
    p = norm.cdf(np.asarray(thr, dtype=np.float32).astype(np.float64))
    za = np.empty(p.shape)
    zh = np.empty(p.shape)
    for k in range(len(pop_off) - 1):
        g = G[:, pop_off[k]:pop_off[k + 1]]
        m = g.shape[1]
        h = 2.0 * p[:, k] * (1.0 - p[:, k])
        za[:, k] = (g.sum(axis=1, dtype=np.int64) / (2.0 * m) - p[:, k]) / np.sqrt(p[:, k] * (1.0 - p[:, k]) / (2.0 * m))
        zh[:, k] = ((g == 1).sum(axis=1) / float(m) - h) / np.sqrt(h * (1.0 - h) / m)
    return za, zh


def adjacent_correlation(G, pop_off):
    """Pearson correlation of the genotypes of SNP s and SNP s - 1 inside every population: (n_snp - 1, n_pop)."""
    pop_off = np.asarray(pop_off, dtype=np.int64)
    out = np.empty((G.shape[0] - 1, len(pop_off) - 1))
    for k in range(len(pop_off) - 1):
        g = G[:, pop_off[k]:pop_off[k + 1]].astype(np.float64)
        g = g - g.mean(axis=1, keepdims=True)
        sd = np.sqrt((g * g).sum(axis=1))
        out[:, k] = (g[1:] * g[:-1]).sum(axis=1) / (sd[1:] * sd[:-1])
    return out
