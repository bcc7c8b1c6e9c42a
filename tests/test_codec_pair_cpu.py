"""The hand-over ring between the codec transformer and SEANet (tr_out, 4 frame slots) as a pure-Python mirror of the rule in
pocket_tts_amd/csrc: which slots a transformer launch of one frame or of a pair writes (GemmArgs::yring), which slots SEANet
frame f reads (GemmArgs::xmask = 3: f and the slot before it), which zq half a launch reads and writes (the launch counter's
parity), and what mimi_parts_check admits.  Checked for every start parity and every mix of singles and pairs up to 12 frames:
no slot that a waiting SEANet frame still reads is overwritten, every frame is read from the slot it was written to, and its
halo is the frame before it.  No GPU."""

import itertools

SLOTS = 4


def tr_writes(n, frames):
    """slots written by a transformer launch whose first frame is n: row tile mt of a pair goes to (n + (mt & 1)) & 3"""
    return [(n + k) & (SLOTS - 1) for k in range(frames)]


def seanet_reads(f):
    """(current, previous) slot of SEANet frame f: par = f & 3, previous = (par - 1) & 3"""
    par = f & (SLOTS - 1)
    return par, (par - 1) & (SLOTS - 1)


def admitted(h_tr, h_frame, frames):
    """mimi_parts_check for a transformer launch: the waiting frames, the halo of the oldest and the new frames fit the ring"""
    return (h_tr - h_frame) + frames + 1 <= SLOTS


def mixes(total):
    """every sequence of 1s and 2s that sums to `total`"""
    if total == 0:
        yield ()
    for k in (1, 2):
        if k <= total:
            for rest in mixes(total - k):
                yield (k,) + rest


class Ring:
    def __init__(self, start):
        self.h_tr = self.h_frame = start  # frames before `start` were decoded whole
        self.slot = {(start - 1) & 3: start - 1}  # what each slot holds: the frame before the first is the first's halo
        self.launches = 0
        self.zq = {1: "prev"}  # zq halves by launch parity: the half a launch READS is (launches & 1) ^ 1

    def tr(self, frames):
        assert admitted(self.h_tr, self.h_frame, frames)
        waiting = range(self.h_frame, self.h_tr)
        live = {s for f in waiting for s in seanet_reads(f)} | {(self.h_tr - 1) & 3}  # + the halo of the first new frame
        for k, s in enumerate(tr_writes(self.h_tr, frames)):
            assert s not in live, (self.h_tr, frames, s, sorted(live))
            self.slot[s] = self.h_tr + k
            live.add(s)
        par = self.launches & 1
        assert self.zq.get(par ^ 1) == ("prev" if self.launches == 0 else self.h_tr - 1)  # the carry of the launch's FIRST frame
        self.zq[par] = self.h_tr + frames - 1  # a pair stores its second frame's vector only
        self.launches += 1
        self.h_tr += frames

    def seanet(self):
        f = self.h_frame
        assert f < self.h_tr
        cur, prev = seanet_reads(f)
        assert self.slot[cur] == f and self.slot[prev] == f - 1, (f, self.slot)
        self.h_frame += 1


def test_every_mix_in_pipeline_order():
    """the pipeline's order: a transformer launch, then the SEANet frames it feeds, then the next launch"""
    n_mixes = 0
    for start in range(4):
        for total in range(1, 13):
            for mix in mixes(total):
                r = Ring(start)
                for frames in mix:
                    r.tr(frames)
                    for _ in range(frames):
                        r.seanet()
                assert r.h_frame == r.h_tr == start + total
                n_mixes += 1
    assert n_mixes == 4 * sum(len(list(mixes(t))) for t in range(1, 13))


def test_every_admitted_interleaving_is_safe():
    """any order of launches that mimi_parts_check admits: the transformer may run ahead of SEANet as far as the ring allows"""
    for start in range(4):
        for ops in itertools.product((1, 2, "s"), repeat=7):
            r = Ring(start)
            for op in ops:
                if op == "s":
                    if r.h_frame < r.h_tr:
                        r.seanet()
                elif admitted(r.h_tr, r.h_frame, op):
                    r.tr(op)


def test_what_the_rule_admits():
    assert admitted(0, 0, 2) and admitted(1, 0, 2) and not admitted(2, 0, 2)  # a pair beside at most one waiting frame
    assert admitted(2, 0, 1) and not admitted(3, 0, 1)                        # a single beside at most two
    for f in range(8):
        assert seanet_reads(f) == (f % 4, (f - 1) % 4)
    assert tr_writes(3, 2) == [3, 0] and tr_writes(6, 1) == [2]
