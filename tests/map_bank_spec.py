"""The map bank's selection rule and validity predicates (include/track2d_bank.h) in plain Python: what the tests hold the
library's generator kernels, t2d_map_bank_index and t2d_map_bank_attach to.

    CYCLE    idx = (genv + ep) mod K
    RANDOM   idx = bounded(K - 1) over the words of the episode's MAP stream: word i is component (i & 3) of
             philox4x32_10(counter (i >> 2, ep, genv, 0), key (seed & 0xffffffff, seed >> 32)); bounded(m) masks a word with the
             smallest 2^b - 1 >= m and takes words from i = 0 until the masked word is <= m; K = 1 draws nothing.
"""
import numpy as np

from draw_spec import philox4x32_10

CYCLE, RANDOM = 0, 1
SELECT = {"cycle": CYCLE, "random": RANDOM}
STREAM_MAP = 0
MIN_FREE = 3
MAX_MAPS = 65536


def map_word(seed, genv, ep, i):
    """Word i of the MAP stream of episode `ep` of global env `genv`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32_10((i >> 2, int(ep), int(genv), STREAM_MAP), (seed & 0xFFFFFFFF, seed >> 32))
    return int(out[i & 3])


def bounded(words, m):
    """Masked rejection over the word sequence `words` (a callable i -> word): (value in [0, m], words used)."""
    if m == 0:
        return 0, 0
    mask = (1 << int(m).bit_length()) - 1
    i = 0
    while True:
        v = words(i) & mask
        i += 1
        if v <= m:
            return v, i


def index(select, seed, genv, ep, count):
    genv, ep = int(genv) & 0xFFFFFFFF, int(ep) & 0xFFFFFFFF
    if select == CYCLE:
        return (genv + ep) % count
    return bounded(lambda i: map_word(seed, genv, ep, i), count - 1)[0]


def indices(select, seed, env_id_base, episodes, count):
    """int32 [N]: the bank index of env e in episode episodes[e] — index() for every env at once (the same rule on arrays:
    each env keeps the first word of its stream whose masked value is <= K - 1)."""
    ep = np.asarray(episodes, np.uint64) & np.uint64(0xFFFFFFFF)
    genv = (np.arange(len(ep), dtype=np.uint64) + np.uint64(int(env_id_base))) & np.uint64(0xFFFFFFFF)
    if select == CYCLE:
        return ((genv + ep) % np.uint64(count)).astype(np.int32)
    out = np.zeros(len(ep), np.int32)
    if count == 1:
        return out
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    m, mask = count - 1, (1 << int(count - 1).bit_length()) - 1
    open_ = np.ones(len(ep), bool)
    i = 0
    while open_.any():
        words = philox4x32_10((np.full(len(ep), i >> 2, np.uint64), ep, genv, STREAM_MAP), (seed & 0xFFFFFFFF, seed >> 32))[i & 3]
        v = words.astype(np.int64) & mask
        take = open_ & (v <= m)
        out[take] = v[take]
        open_ &= ~take
        i += 1
    return out


def rejections(seed, genv, ep, count):
    """Words the RANDOM rule discards before it accepts one."""
    return bounded(lambda i: map_word(seed, genv, ep, i), count - 1)[1] - 1 if count > 1 else 0


def map_ok(m):
    """Cells 0 / 1, an all-wall border, at least three free cells."""
    m = np.asarray(m)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or ((m != 0) & (m != 1)).any():
        return False
    if not (m[0].all() and m[-1].all() and m[:, 0].all() and m[:, -1].all()):
        return False
    return int((m == 0).sum()) >= MIN_FREE


def spawn_ok(m, row):
    """All -1, or two free in-map cells (they may coincide)."""
    row = [int(v) for v in row]
    if row == [-1] * 4:
        return True
    side = m.shape[0]
    if any(v < 0 or v >= side for v in row):
        return False
    return m[row[0], row[1]] == 0 and m[row[2], row[3]] == 0
