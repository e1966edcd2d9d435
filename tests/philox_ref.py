"""numpy restatement of the draw scheme of ``anr_train_ray_sample`` (include/aninerf.h): Philox4x32-10
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; constants of the
Random123 library), and ``PhiloxDraws``, an ``rng`` for ``oracle.restate.sample_ray_train`` /
``data.sample_ray_h36m`` that hands out the device sampler's draws in the reference's call order."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (2,) of 32-bit words -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & _MASK, int(key[1]) & _MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_MASK)]
        k0, k1 = (k0 + W0) & _MASK, (k1 + W1) & _MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def slot_words(seed, step, rnd, lo, hi):
    """The 32-bit draw of slots lo..hi-1 of round ``rnd``: word i & 3 at counter (i >> 2, rnd, step)."""
    i = np.arange(lo, hi, dtype=np.uint64)
    ctr = np.stack([i >> np.uint64(2), np.full_like(i, rnd), np.full_like(i, step & _MASK),
                    np.full_like(i, (step >> 32) & _MASK)], axis=-1)
    w = philox4x32_10(ctr, (seed & _MASK, (seed >> 32) & _MASK))
    return w[np.arange(len(i)), (i & np.uint64(3)).astype(np.int64)]


class PhiloxDraws:
    """``randint(0, n, size)`` as the sampling loop calls it: ``calls_per_round`` calls make a round
    (3: body, face, bound; 2 where the face list is empty and the reference skips that call), each
    call takes the next ``size`` slots of the round. ``rounds`` counts the rounds begun and
    ``round_slots[r]`` the slots round r handed out."""

    def __init__(self, seed, step, calls_per_round=3):
        self.seed, self.step, self.calls_per_round = int(seed), int(step), int(calls_per_round)
        self.round_slots = []
        self._call = 0

    @property
    def rounds(self):
        return len(self.round_slots)

    def randint(self, lo, hi, size):
        assert lo == 0
        if hi <= 0:
            raise ValueError('low >= high')  # np.random.randint(0, 0, n)
        if self._call == 0:
            self.round_slots.append(0)
        r, first = len(self.round_slots) - 1, self.round_slots[-1]
        x = slot_words(self.seed, self.step, r, first, first + int(size)).astype(np.uint64)
        self.round_slots[-1] = first + int(size)
        self._call = (self._call + 1) % self.calls_per_round
        return ((x * np.uint64(hi)) >> np.uint64(32)).astype(np.int64)
