"""The region table of k_lookup_v5's exact stage 1 (gm_region_table.h) on a host model: its inserts are single-shot atomics -- one compare-and-swap claims a slot, whose tag
never changes again, then OR for the flags and MAX for min / max -- so what the table holds does not depend on the order in which the candidates' operations arrive.  That is
why no barrier has to stand between step (a), every candidate's try at the first slot of its region's probe sequence, and step (b), the probe-ons and the strip marks: a
wave works its own list of (b) off while other waves are still in (a).  Here every atomic is one step of a generator, and the same candidates run in today's order, wave by
wave, and with the waves' operation sequences interleaved at random."""
import numpy as np
import pytest

FA, FB, FC, FD, FE = 1, 2, 4, 8, 16
M32 = 0xFFFFFFFF
WAVE = 64


class Table:
    def __init__(self, hbits):
        self.hbits, self.hmask, self.hshift = hbits, (1 << hbits) - 1, 32 - hbits
        self.htag = [0] * (1 << hbits); self.hmin = [0] * (1 << hbits); self.hmax = [0] * (1 << hbits)
        self.slot_of = {}                                        # candidate -> slot (what settle leaves in candp[])

    @staticmethod
    def mul24(a, c):
        return ((a & 0xFFFFFF) * (c & 0xFFFFFF)) & M32

    def hash(self, r1):
        return self.mul24(r1, 0x9E3779) >> self.hshift

    def step(self, r1):
        return (self.mul24(r1, 0x7FEB35) >> 7) | 1

    # Every generator yields BEFORE each atomic operation: between two yields exactly one atomic happens.
    def cas(self, h, new):
        yield
        prev = self.htag[h]
        if prev == 0: self.htag[h] = new
        return prev

    def fetch_or(self, h, m):
        yield
        old = self.htag[h]; self.htag[h] = old | m
        return old

    def again(self, h, prev, own):                               # k5_again
        first = (FA | FC) if own else FA
        old = prev
        if (old & first) != first: old = yield from self.fetch_or(h, first)
        need = (FB if old & FA else 0) | (FD if own and old & FC else 0) | (FE if own and old & FD else 0)
        need &= ~old
        if need:
            old2 = yield from self.fetch_or(h, need)
            if own and (need & FD) and (old2 & FD) and not (old2 & FE): yield from self.fetch_or(h, FE)

    def insert(self, r, own, second=False):                      # k5_insert
        r1 = r + 1; t = r1 << 8; first = (FA | FC) if own else FA
        h = self.hash(r1); st = self.step(r1)
        if second: h = (h + st) & self.hmask
        for _ in range(self.hmask + 1):
            prev = yield from self.cas(h, t | first)
            if prev == 0: return h
            if (prev >> 8) == r1:
                yield from self.again(h, prev, own)
                return h
            h = (h + st) & self.hmask
        return None

    def settle(self, i, h, off):                                 # two MAX operations
        yield
        self.hmin[h] = max(self.hmin[h], 0x10000 - off)
        yield
        self.hmax[h] = max(self.hmax[h], off + 1)
        self.slot_of[i] = h

    def first_try(self, i, r, off, deferred):                    # step (a) of candidate i; a miss goes to `deferred`, a hit in the overlap strip leaves a strip mark there
        r1 = r + 1; h0 = self.hash(r1)
        prev = yield from self.cas(h0, (r1 << 8) | FA | FC)
        if prev == 0 or (prev >> 8) == r1:
            if prev != 0: yield from self.again(h0, prev, True)
            yield from self.settle(i, h0, off)
            if off < OVL and r > 0: deferred.append(("mark", r - 1))
        else:
            deferred.append(("cand", i, r, off))

    def later(self, item):                                       # step (b): probe_on / a strip mark
        if item[0] == "mark":
            h = yield from self.insert(item[1], False)
            assert h is not None
            return
        _, i, r, off = item
        h = yield from self.insert(r, True, True)
        assert h is not None
        yield from self.settle(i, h, off)
        if off < OVL and r > 0:
            h = yield from self.insert(r - 1, False)
            assert h is not None

    def contents(self):
        out = {}
        for h, t in enumerate(self.htag):
            if t:
                r = (t >> 8) - 1
                assert r not in out, "region %d sits in two slots" % r
                out[r] = (t & 0xFF, self.hmin[h], self.hmax[h])
        return out


OVL = 9
RB = 6


def run(g):
    for _ in g: pass


def wave_ops(T, cands, lo, hi):
    """one wave: step (a) of its candidates, then its own list of step (b), the strip marks behind the deferred candidates"""
    deferred = []
    for i in range(lo, hi):
        yield from T.first_try(i, cands[i][0], cands[i][1], deferred)
    for item in [d for d in deferred if d[0] == "cand"] + [d for d in deferred if d[0] == "mark"]:
        yield from T.later(item)


def order_today(T, cands):
    deferred = []
    for i, (r, off) in enumerate(cands): run(T.first_try(i, r, off, deferred))
    for item in [d for d in deferred if d[0] == "cand"] + [d for d in deferred if d[0] == "mark"]: run(T.later(item))


def order_wave_by_wave(T, cands):
    for lo in range(0, len(cands), WAVE): run(wave_ops(T, cands, lo, min(lo + WAVE, len(cands))))


def order_interleaved(T, cands, rng):
    live = [wave_ops(T, cands, lo, min(lo + WAVE, len(cands))) for lo in range(0, len(cands), WAVE)]
    while live:
        k = int(rng.integers(len(live)))
        try: next(live[k])
        except StopIteration: live.pop(k)


def draw(rng, n_regions):
    """about 400 candidates over n_regions distinct regions (their strip marks' regions included): three regions with 40+ candidates, forty pairs, singles; distinct positions"""
    nreg = 1 << 16
    regs = rng.choice(np.arange(1, nreg - 1), size=n_regions, replace=False)
    cands = set()
    for r in regs[:3]:
        for off in rng.choice(1 << RB, size=int(rng.integers(40, 50)), replace=False): cands.add((int(r), int(off)))
    for r in regs[3:43]:
        for off in rng.choice(1 << RB, size=2, replace=False): cands.add((int(r), int(off)))
    used = {r for r, _ in cands} | {r - 1 for r, off in cands if off < OVL}
    for r in regs[43:]:
        if len(used) >= n_regions: break
        # every fourth single sits in the overlap strip: its mark goes to the region before
        off = int(rng.integers(0, OVL)) if rng.integers(4) == 0 else int(rng.integers(OVL, 1 << RB))
        new = {int(r)} | ({int(r) - 1} if off < OVL else set())
        if len(used | new) > n_regions: continue
        cands.add((int(r), off)); used |= new
    cands = sorted(cands)
    rng.shuffle(cands)
    return [tuple(c) for c in cands], len(used)


def direct_count(cands):
    marks, inside, lo, hi = {}, {}, {}, {}
    for r, off in cands:
        marks[r] = marks.get(r, 0) + 1; inside[r] = inside.get(r, 0) + 1
        lo[r] = min(lo.get(r, off), off); hi[r] = max(hi.get(r, off), off)
        if off < OVL and r > 0: marks[r - 1] = marks.get(r - 1, 0) + 1
    out = {}
    for r, m in marks.items():
        n = inside.get(r, 0)
        fl = FA | (FB if m >= 2 else 0) | (FC if n >= 1 else 0) | (FD if n >= 2 else 0) | (FE if n >= 3 else 0)
        out[r] = (fl, 0x10000 - lo[r] if n else 0, hi[r] + 1 if n else 0)
    return out


@pytest.mark.parametrize("hbits,load", [(10, 1.0 / 3.0), (8, 0.9)], ids=["a_third_full", "ninety_percent_full"])
def test_table_contents_do_not_depend_on_the_order_of_the_atomics(hbits, load):
    rng = np.random.Generator(np.random.PCG64(16))
    for trial in range(20):
        cands, n_distinct = draw(rng, int(load * (1 << hbits)))
        assert 330 <= len(cands) <= 520 and abs(n_distinct - load * (1 << hbits)) <= 2, (len(cands), n_distinct)
        want = direct_count(cands)
        assert sum(1 for v in want.values() if v[0] & FE) >= 3 and any(not (v[0] & FC) for v in want.values())      # (crowded regions and mark-only regions are both there)
        tables = []
        for way in range(3):
            T = Table(hbits)
            if way == 0: order_today(T, cands)
            elif way == 1: order_wave_by_wave(T, cands)
            else: order_interleaved(T, cands, rng)
            got = T.contents()                                   # (asserts that no region sits in two slots)
            assert got == want, (trial, way, {r: (got.get(r), want.get(r)) for r in set(got) | set(want) if got.get(r) != want.get(r)})
            assert len(T.slot_of) == len(cands)
            for i, (r, off) in enumerate(cands):
                assert (T.htag[T.slot_of[i]] >> 8) - 1 == r, (trial, way, i)
            tables.append(got)
        assert tables[0] == tables[1] == tables[2]
