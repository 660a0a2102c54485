"""Synthetic text generators."""
import numpy as np

_M = (1 << 64) - 1


def splitmix64_stream(n, seed):
    """n outputs of splitmix64 with state starting at `seed` (vectorised)."""
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        x = np.uint64(seed & _M) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dna(n, seed):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return lut[(splitmix64_stream(n, seed) & np.uint64(3)).astype(np.int64)]


def ascii128(n, seed):
    return (splitmix64_stream(n, seed) & np.uint64(127)).astype(np.uint8)


def bytes_mod127p1(n, seed):
    return (1 + splitmix64_stream(n, seed) % np.uint64(127)).astype(np.uint8)


def tandem(n, period, unit):
    unit = np.asarray(unit, dtype=np.uint8)
    assert unit.size == period
    reps = (n + period - 1) // period
    return np.tile(unit, reps)[:n].copy()


def cyclic(n, word):
    w = np.frombuffer(word.encode(), dtype=np.uint8)
    return np.tile(w, (n + w.size - 1) // w.size)[:n].copy()


def mutated(n, period, seed):
    """TANDEM(n, period, seed) with one position in 200 given a character of its own (psacx_synth_text_dev kind 3):
    position g is mutated when the g-th output of the stream seeded seed ^ 0xA5A5A5A5A5A5A5A5 is a multiple of 200."""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = tandem(n, period, dna(period, seed))
    m = splitmix64_stream(n, seed ^ 0xA5A5A5A5A5A5A5A5)
    hit = (m % np.uint64(200)) == 0
    t[hit] = lut[((m[hit] >> np.uint64(8)) & np.uint64(3)).astype(np.int64)]
    return t


# Value arrays at the edges of the key width, for the ANSV tests (tests/test_gpu_kernel_edges.py on the GPU, tests/test_oracle_golden.py
# pins the oracle on the same shapes).  MAX = 2^bits - 1 is also what the kernels pad with.
ANSV_EDGE_SHAPES = ("uniform", "top3", "max", "falling", "rising", "deep")
ANSV_EDGE_SHAPES_64 = ("low_zero", "high_equal", "halves")      # a 64-bit value travels between lanes as two halves


def ansv_edge_values(shape, n, dtype, seed=1):
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    mx = (1 << bits) - 1
    rng = np.random.RandomState(seed)
    full = (splitmix64_stream(n, seed * 7919 + n) >> np.uint64(64 - bits)).astype(dt)
    i = np.arange(n, dtype=np.uint64)
    if shape == "uniform":
        return full
    if shape == "top3":                          # {MAX - 2, MAX - 1, MAX}
        return (np.uint64(mx) - rng.randint(0, 3, size=n).astype(np.uint64)).astype(dt)
    if shape == "max":
        return np.full(n, mx, dt)
    if shape == "falling":                       # strictly falling from MAX
        return (np.uint64(mx) - i).astype(dt)
    if shape == "rising":                        # strictly rising, the last element is MAX
        return (np.uint64(mx - (n - 1)) + i).astype(dt)
    if shape == "deep":                          # answers many tiles away: about one element in 10^4 is 0
        v = full.copy()
        v[rng.rand(n) < 1e-4] = 0
        return v
    assert bits == 64, shape
    r = rng.randint(0, 32, size=n).astype(np.uint64) * np.uint64(0x08000001)        # 32 values that spread over a 32-bit half
    if shape == "low_zero":
        return r << np.uint64(32)
    if shape == "high_equal":
        return (np.uint64(7) << np.uint64(32)) | r
    if shape == "halves":                        # neighbours differ in one half only, the halves taking turns
        hi = (rng.randint(0, 5, size=n // 2 + 2).astype(np.uint64) * np.uint64(0x30000001))[((i + np.uint64(1)) // np.uint64(2)).astype(np.int64)]
        lo = (rng.randint(0, 5, size=n // 2 + 2).astype(np.uint64) * np.uint64(0x30000001))[(i // np.uint64(2)).astype(np.int64)]
        return (hi << np.uint64(32)) | lo
    raise ValueError(shape)
