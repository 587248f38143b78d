"""Restatement of simulateLD's draws (simulateLD.cpp:134-151) for the tests: numpy.random.RandomState(seed) gives the raw uint32
stream of std::mt19937(seed); uniform_int_distribution<>(0, n - 1) is libstdc++'s Lemire draw on a 64-bit product."""
import numpy as np


def counts(weights, sim_size):
    """(int)(w * sim_size) in fp64 on the raw weight."""
    return [int(float(w) * float(sim_size)) for w in weights]


def draws(seed, sizes, cnts):
    """[(q, s)] for populations with `sizes` and `cnts` draws each, in that order, on one generator."""
    rs = np.random.RandomState(seed)
    buf, pos = np.zeros(0, dtype=np.uint64), 0

    def nxt():
        nonlocal buf, pos
        if pos == len(buf):
            buf, pos = rs.randint(0, 2 ** 32, size=4096, dtype=np.uint32).astype(np.uint64), 0
        pos += 1
        return int(buf[pos - 1])

    out = []
    for q, (n, c) in enumerate(zip(sizes, cnts)):
        n, c = int(n), int(c)
        for _ in range(c):
            prod = nxt() * n
            low = prod & 0xFFFFFFFF
            if low < n:
                thr = (2 ** 32 - n) % n
                while low < thr:
                    prod = nxt() * n
                    low = prod & 0xFFFFFFFF
            out.append((q, prod >> 32))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def gathered(G, pop_off, dr, n_cols):
    """The reference's geno_mat: columns of G [S, N] (codes) picked by the draws, then n_cols - n_drawn zero columns."""
    G = np.asarray(G)
    po = np.asarray(pop_off)
    cols = po[dr[:, 0]] + dr[:, 1] if len(dr) else np.zeros(0, dtype=np.int64)
    out = np.zeros((G.shape[0], int(n_cols)), dtype=np.uint8)
    out[:, :len(cols)] = G[:, cols]
    return out
