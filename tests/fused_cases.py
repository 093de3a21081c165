"""The fused check batch's term scalars as Python integers, and the records that go with them: shared by
tests/test_fused_lane_host.py (csrc/fused_lane.hpp compiled for the CPU under ASan + UBSan) and tests/test_gpu_check_fused.py
(k_fused_terms on the device).  A record is a member's xi_0 .. xi_lg | z | v | c | r | s, Montgomery words (x 2^256 mod r); its
2 lg + 2 scalars are r | r xi_1^-1 .. r xi_lg^-1 | r xi_1 .. r xi_lg | s - r c and its share of H's scalar r (v - c h(z)) xi_0,
canonical integers below r."""
import random

import numpy as np

R_MOD = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
MONT = (1 << 256) % R_MOD
SPECIAL_XI = (1, R_MOD - 1, (1 << 254) % R_MOD)
SPECIAL_C = (0, 1, R_MOD - 1)
SPECIAL_W = (0, 1, R_MOD - 1)


def words(x):
    """a 256-bit integer as 4 little-endian 64-bit words"""
    return [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def from_words(w):
    return sum(int(w[k]) << (64 * k) for k in range(4))


class Member:
    """one member's inputs as integers in [0, r)"""

    def __init__(self, xis, z, v, c, r, s):
        self.xis, self.z, self.v, self.c, self.r, self.s = list(xis), z, v, c, r, s
        self.lg = len(self.xis) - 1

    def record(self):
        vals = self.xis + [self.z, self.v, self.c, self.r, self.s]
        return np.array([w for x in vals for w in words(x * MONT % R_MOD)], dtype=np.uint64)

    def hz(self):
        """HPoly::eval: prod_k (1 + xi_(lg - k) z^(2^k))"""
        acc, zi = 1, self.z
        for k in range(self.lg):
            acc = acc * (1 + self.xis[self.lg - k] * zi) % R_MOD
            zi = zi * zi % R_MOD
        return acc

    def scalars(self):
        inv = [pow(x, -1, R_MOD) if x else 0 for x in self.xis[1:]]
        return ([self.r] + [self.r * i % R_MOD for i in inv] + [self.r * x % R_MOD for x in self.xis[1:]]
                + [(self.s - self.r * self.c) % R_MOD])

    def share(self):
        return self.r * (self.v - self.c * self.hz()) % R_MOD * self.xis[0] % R_MOD


def members(lg, count, seed):
    """`count` members at lg: the special values of the challenges, of c, of the weights and z = 0 first (each in turn in an
    otherwise random member, then all at once), random ones behind"""
    rng = random.Random(1000 * lg + seed)
    rnd = lambda: rng.randrange(1, R_MOD)
    out = []

    def member(**kw):
        m = Member([rnd() for _ in range(lg + 1)], rnd(), rnd(), rnd(), rnd(), rnd())
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    for x in SPECIAL_XI:
        out.append(member(xis=[x] * (lg + 1)))                       # every challenge the special value
        out.append(member(xis=[rnd() for _ in range(lg)] + [x]))     # ... the last one alone
        out.append(member(xis=[x] + [rnd() for _ in range(lg)]))     # ... xi_0 alone
    for c in SPECIAL_C:
        out.append(member(c=c))
    out.append(member(z=0))
    for r in SPECIAL_W:
        for s in SPECIAL_W:
            out.append(member(r=r, s=s))
    out.append(Member([R_MOD - 1] * (lg + 1), 0, R_MOD - 1, R_MOD - 1, R_MOD - 1, R_MOD - 1))
    out.append(member(v=0, c=0))
    while len(out) < count:
        out.append(member())
    rng.shuffle(out)
    return out[:count] if count < len(out) else out


def check_member(m, got_scalars, got_share):
    """got_scalars: (2 lg + 2, 4) words, got_share: 4 words -> list of (what, index) that differ"""
    bad = []
    for k, want in enumerate(m.scalars()):
        if [int(w) for w in got_scalars[k]] != words(want):
            bad.append(("scalar", k))
    if got_share is not None and [int(w) for w in got_share] != words(m.share()):
        bad.append(("share", 0))
    return bad
