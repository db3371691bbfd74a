"""The random background colour of a training batch (--random_bg) restated in NumPy with uint64
arithmetic: the definition the draw kernel (csrc/data.hip, mfnerf_sample_rays_prep_bg) is held to.

    key        = splitmix64(splitmix64(seed ^ BG_STREAM) ^ call)
    colour[c]  = (mix32(key + c * GOLDEN) >> 8) * 2^-24,  c = 0, 1, 2      -- U[0,1) with 24 bits

`call` is the dataset's draw counter as the launch reads it (the number of draws made before).
BG_STREAM is the colour's own stream constant, distinct from the two of the ray and noise draws."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BG_STREAM = np.uint64(0xA0761D6478BD642F)
RAY_STREAM, NOISE_STREAM = np.uint64(0xD1B54A32D192ED03), np.uint64(0x8CB92BA72F3D8DD7)  # csrc/data.hip draw_ray


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = _u64(x) + GOLDEN
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mix32(x):
    """The low 32 bits of the murmur3 64-bit finaliser."""
    with np.errstate(over="ignore"):
        x = _u64(x)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xFF51AFD7ED558CCD)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xC4CEB9FE1A85EC53)
        x = x ^ (x >> np.uint64(33))
        return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def bg_colour(seed, call):
    """-> (3,) float32, or (n, 3) for an array of calls.  seed: the dataset's seed (a Python int,
    taken modulo 2^64 as the C ABI's uint64_t takes it)."""
    seed = np.uint64(int(seed) % (1 << 64))
    call = _u64(call)
    key = splitmix64(splitmix64(seed ^ BG_STREAM) ^ call)
    with np.errstate(over="ignore"):
        k = key[..., None] + np.arange(3, dtype=np.uint64) * GOLDEN
    bits = mix32(k) >> np.uint32(8)
    return (bits.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
