"""numpy float64 references of the softmax passes (rails_amd/csrc/softmax.hip): the log-partition with its special rows,
an integer-exact Philox4x32-10, the Gumbel transform and the perturbed matrix."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # Philox4x32 multipliers (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
W0, W1 = 0x9E3779B9, 0xBB67AE85      # Weyl key increments
MASK32 = np.uint64(0xFFFFFFFF)


def floats(bits):
    """uint32 bit patterns -> float64 values"""
    with np.errstate(invalid="ignore"):      # (a signalling NaN among the patterns)
        return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)


def lse(bits, eligible, beta):
    """(rows,) float64: per row -inf if nothing eligible or -inf alone, NaN with an eligible NaN, otherwise +inf with an eligible +inf,
    otherwise log sum exp(float64(x) * float64(beta)) over the eligible x."""
    x = floats(bits) * float(np.float32(beta))
    eligible = np.broadcast_to(eligible, x.shape)
    out = np.empty(x.shape[0], dtype=np.float64)
    for r in range(x.shape[0]):
        v = x[r][eligible[r]]
        if v.size == 0 or (v == -np.inf).all():
            out[r] = -np.inf
        elif np.isnan(v).any():
            out[r] = np.nan
        elif (v == np.inf).any():
            out[r] = np.inf
        else:
            m = v.max()
            out[r] = m + np.log(np.exp(v - m).sum())
    return out


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two -> the four output words as uint32 arrays; integer arithmetic alone."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [v.astype(np.uint32) for v in c]


def uniform(w):
    """word -> u = ((w >> 9) + 0.5) * 2^-23 in float64 (exact)"""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(seed, rows, n):
    """(len(rows), n) float64: g(seed, row, x) = -log(-log(u)) for the GLOBAL row numbers `rows` and x = 0 .. n - 1"""
    rows = np.asarray(rows, dtype=np.uint64)[:, None]
    x = np.arange(n, dtype=np.uint64)[None, :]
    w = philox4x32_10((x, rows & MASK32, rows >> np.uint64(32), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return -np.log(-np.log(uniform(w)))


def perturbed(bits, eligible, beta, seed, first_row=0):
    """(rows, n) float64: float64(x) * float64(beta) + g on the eligible entries, -inf elsewhere"""
    x = floats(bits) * float(np.float32(beta))
    with np.errstate(invalid="ignore"):
        out = x + gumbel(seed, first_row + np.arange(x.shape[0]), x.shape[1])
    return np.where(np.broadcast_to(eligible, x.shape), out, -np.inf)


def chi_square(logits, temperature, seed, rows):
    """Pearson's statistic of the per-item counts of the row argmax of `rows` identical perturbed rows against softmax(logits / T) -> (chi2,
    the smallest expected count, the argmax per row, the gap between each row's two largest perturbed values)"""
    logits = np.asarray(logits, dtype=np.float32)
    bits = np.broadcast_to(logits.view(np.uint32), (rows, logits.size))
    z = perturbed(bits, True, np.float32(1.0 / temperature), seed)
    arg = z.argmax(axis=1)
    top2 = np.sort(z, axis=1)[:, -2:]
    y = logits.astype(np.float64) * float(np.float32(1.0 / temperature))
    p = np.exp(y - y.max())
    expected = rows * p / p.sum()
    counts = np.bincount(arg, minlength=logits.size)
    return float(((counts - expected) ** 2 / expected).sum()), float(expected.min()), arg, top2[:, 1] - top2[:, 0]
