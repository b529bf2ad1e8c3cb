"""A numpy model of the blocked layout's beam-state store: the double buffers `bk.d_target[0..1]`, `bk.d_last[0..1]`,
`bk.d_plastic[0..1]`, the half `bk.cur` that is current, and what a launch, the export, the beam import, a checkpoint and a restore
read and write of them.  Bookkeeping only: no physics.  Every value is a 32-bit WORD (the kernels move and compare words).

Where each rule comes from (csrc/):
  upload    sb_api.hip:398-417 blocked_state_to_device: target into both halves, last into half 0 (half 1 zeroed), the plastic
            flag of a tile in both rows = some beam it owns has memcmp(length, target_length) != 0; cur = 0.
  launch    sb_blocked.hip:809-810 launch_one: reads half cur, writes half cur ^ 1, also of the plastic rows; :847-848 flips e->cur
            and bk.cur.  k_substep_blocked: :135 own_plastic = plastic_r[tile]; :141-147 nb_plastic = some neighbour's plastic_r;
            :247 / :282 last of own and halo beams from last_r; :262 own targets from target_r only when own_plastic; :281 halo
            targets from target_r only when nb_plastic; :357-365 everything not fetched is the rest length; :554-563 plastic_w =
            own_plastic or some owned beam's target differs from its rest length by bits, stored to plastic_w[tile]; :569 targets
            stored to target_w only when plastic_w; :570 last stored to last_w always.
  export    sb_state_io.hip:216 reads e->beams.target / last, which sb_blocked.hip:891-892 point at half cur -- whatever the flags say.
  import    sb_state_io.hip:113-122 k_state_import_beams_blocked, called with (:316) target_a / target_b = d_target[0] / [1],
            last_cur = d_last[bk.cur], plastic_a / plastic_b = d_plastic[0] / [1]; the flag test `v.x != rest[g]` is on uint32_t.
  checkpoint / restore
            sb_state_io.hip:377-386 sbs_walk_run_state: both target halves, last[bcur], strain, stress, both plastic rows, and the
            particle buffer part[cur]; :425-428 the halves and substeps_done of the checkpoint; :441 the restore walks the
            CHECKPOINT's halves; :449-456 e->cur, substeps_done, bk.cur (and beams.target / last) set back.

The particles are one word per tile, `trace`, double buffered by `pcur` (e->cur): a launch folds everything the tile READ into it, so
that a launch that read a stale target, last length or flag leaves a different word -- on the device: different particle bits.

MUTANTS names the model with one line left out or wrong; tests/test_state_io_model_cpu.py runs the scenarios of
tests/test_gpu_state_io_halves.py over the model and every mutant."""
import hashlib

import numpy as np

TARGET, LAST = 1, 2      # SB_BEAM_TARGET_LENGTH, SB_BEAM_LAST_LENGTH

MUTANTS = {
    "import-no-target_a": "import without the store to target half 0",
    "import-no-target_b": "import without the store to target half 1",
    "import-no-plastic_a": "import without the store to plastic row 0",
    "import-no-plastic_b": "import without the store to plastic row 1",
    "import-last-half0": "import writes last into half 0 instead of half cur",
    "import-last-both": "import writes last into both halves",
    "import-flag-float": "import raises the flag by != on floats instead of on words",
    "ckpt-last0": "checkpoint saves last[0] instead of last[bcur]",
    "ckpt-target-cur-only": "checkpoint saves (and the restore writes) only target[bcur]",
    "restore-no-cur": "restore does not set bk.cur (beams.target / last) back",
    "restore-engine-halves": "restore copies into the halves that are current at the restore, not the checkpoint's",
    "restore-no-plastic": "restore without the plastic rows",
}

# Mutants that no scenario can tell from the model, with the argument from the kernel source.
EQUIVALENT = {
    # The half that is not current is only ever WRITTEN before it becomes current: every launch stores last_w for every beam its
    # tiles own (sb_blocked.hip:570; a removed beam's at :583, copied from last_r), and every read of a last length -- :247, :282,
    # :579, the export, the checkpoint's d_last[bcur] -- is of the current half.  A value the import leaves in the other half is
    # overwritten by the next launch and read by nothing before that.
    "import-last-both",
}


def words(x):
    return np.ascontiguousarray(np.asarray(x, dtype="<f4")).view("<u4").copy()


def floats(w):
    return np.ascontiguousarray(np.asarray(w, dtype="<u4")).view("<f4")


def as_words(x):
    """float32 values as their words; unsigned integers are words already"""
    a = np.asarray(x)
    return a.astype("<u4") if a.dtype.kind == "u" else words(a)


def _fold(*parts):
    h = hashlib.blake2b(digest_size=8)
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return np.frombuffer(h.digest(), "<u8")[0]


class Store:
    """`rest`, `target`, `last`: float32 arrays (or their words) per beam in owner order; `tile_b0`: first beam of each tile and
    the end.  Tiles t - 1 and t + 1 are tile t's neighbours (their beams are its halo)."""

    def __init__(self, rest, target, last, tile_b0, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.m = mutant
        self.rest, up_t, up_l = as_words(rest), as_words(target), as_words(last)
        self.b0 = np.asarray(tile_b0, np.int64)
        self.T, self.B = self.b0.size - 1, self.rest.size
        assert self.b0[0] == 0 and self.b0[-1] == self.B
        self.tile_of = np.repeat(np.arange(self.T), np.diff(self.b0))
        # sb_api.hip:401-417
        self.target = [up_t.copy(), up_t.copy()]
        self.last = [up_l.copy(), np.zeros(self.B, "<u4")]
        self.strain = np.zeros(self.B, "<u4")
        self.stress = np.zeros(self.B, "<u4")
        pl = np.array([(self.rest[self._own(t)] != up_t[self._own(t)]).any() for t in range(self.T)], "<u4")
        self.plastic = [pl.copy(), pl.copy()]
        self.cur = 0
        self.pcur = 0
        self.trace = [np.zeros(self.T, "<u8"), np.zeros(self.T, "<u8")]
        self.substeps_done = 0
        self.ck = None

    def _own(self, t):
        return slice(int(self.b0[t]), int(self.b0[t + 1]))

    def _halo(self, t):
        nb = [n for n in (t - 1, t + 1) if 0 <= n < self.T]
        return nb, np.concatenate([np.arange(self.b0[n], self.b0[n + 1]) for n in nb])

    # ---- one launch (k_substep_blocked through launch_one)
    def launch(self, new_last, yield_tiles=()):
        """`new_last`: the words the launch leaves as last length of every beam; `yield_tiles`: the tiles in which a beam yields
        (the first beam the tile owns moves its target by a bit pattern that depends on the target the tile saw)."""
        new_last = np.asarray(new_last, "<u4")
        c, o, pc, po = self.cur, self.cur ^ 1, self.pcur, self.pcur ^ 1
        t_r, l_r, p_r = self.target[c], self.last[c], self.plastic[c]
        t_w, l_w, p_w = self.target[o], self.last[o], self.plastic[o]
        for t in range(self.T):
            own = self._own(t)
            nb, halo = self._halo(t)
            own_plastic = p_r[t] != 0                                               # :135
            nb_plastic = any(p_r[n] != 0 for n in nb)                               # :141-147
            seen_own = t_r[own].copy() if own_plastic else self.rest[own].copy()    # :262, :357-365
            seen_halo = t_r[halo] if nb_plastic else self.rest[halo]                # :281, :357-365
            tg = seen_own.copy()
            if t in yield_tiles:
                tg[0] = (int(tg[0]) + 0x1000) & 0xFFFFFFFF
            plastic_w = own_plastic or bool((tg != self.rest[own]).any())           # :554-562
            p_w[t] = 1 if plastic_w else 0                                          # :563
            if plastic_w:
                t_w[own] = tg                                                       # :569
            l_w[own] = new_last[own]                                                # :570
            self.strain[own] = tg ^ new_last[own]                                   # (single buffered: d_strain / d_stress)
            self.stress[own] = tg + new_last[own]
            self.trace[po][t] = _fold(self.trace[pc][t], seen_own, seen_halo, l_r[own], l_r[halo])   # :247, :282
        self.cur, self.pcur = o, po                                                 # :847-848
        self.substeps_done += 1

    # ---- export (sb_state_io.hip:54, :216) and what info "plastic_tiles" counts (sb_api.hip: d_plastic[bk.cur])
    def export(self):
        return np.stack([self.target[self.cur], self.last[self.cur], self.strain, self.stress], axis=1).copy()

    def plastic_tiles(self):
        return int((self.plastic[self.cur] != 0).sum())

    def read(self):
        """everything a read-back on the device shows: the beam rows, the particles, the flag count, the halves, the substep count"""
        return (self.export().tobytes(), self.trace[self.pcur].tobytes(), self.plastic_tiles(), self.cur, self.pcur, self.substeps_done)

    # ---- import (k_state_import_beams_blocked, sb_state_io.hip:113-122)
    def import_beams(self, rows, fields=TARGET | LAST):
        """`rows`: (B, 2) words {target_length, last_length} in owner order"""
        rows = np.asarray(rows, "<u4")
        vt, vl = rows[:, 0], rows[:, 1]
        if fields & TARGET:
            if self.m != "import-no-target_a":
                self.target[0][:] = vt                                              # :114
            if self.m != "import-no-target_b":
                self.target[1][:] = vt                                              # :115
            if self.m == "import-flag-float":
                with np.errstate(invalid="ignore"):
                    differs = floats(vt) != floats(self.rest)
            else:
                differs = vt != self.rest                                           # :116 (uint32_t operands)
            for t in np.unique(self.tile_of[differs]):
                if self.m != "import-no-plastic_a":
                    self.plastic[0][t] = 1                                          # :118
                if self.m != "import-no-plastic_b":
                    self.plastic[1][t] = 1                                          # :119
        if fields & LAST:
            if self.m == "import-last-half0":
                self.last[0][:] = vl
            elif self.m == "import-last-both":
                self.last[0][:] = vl
                self.last[1][:] = vl
            else:
                self.last[self.cur][:] = vl                                         # :122 with :316's d_last[k.cur]

    # ---- checkpoint / restore (sbs_walk_run_state and its two callers)
    def _walk(self, pcur, bcur, saving):
        """(holder, key) of every array of the run state, for the halves named"""
        items = [(self.trace, pcur)]                                                # part[cur]: :371-374
        if self.m == "ckpt-target-cur-only":
            items += [(self.target, bcur)]
        else:
            items += [(self.target, 0), (self.target, 1)]                           # :379-380
        items += [(self.last, 0 if (self.m == "ckpt-last0" and saving) else bcur)]  # :381
        items += [(self, "strain"), (self, "stress")]                               # :382-383
        if not (self.m == "restore-no-plastic" and not saving):
            items += [(self.plastic, 0), (self.plastic, 1)]                         # :384-385
        return items

    @staticmethod
    def _get(holder, key):
        return getattr(holder, key) if isinstance(key, str) else holder[key]

    def checkpoint(self):
        items = self._walk(self.pcur, self.cur, True)                               # :406
        self.ck = dict(data=[self._get(h, k).copy() for h, k in items], pcur=self.pcur, bcur=self.cur,   # :425-428
                       substeps_done=self.substeps_done)

    def restore(self):
        ck = self.ck
        assert ck is not None
        if self.m == "restore-engine-halves":
            items = self._walk(self.pcur, self.cur, False)
        else:
            items = self._walk(ck["pcur"], ck["bcur"], False)                       # :441
        data = ck["data"]
        if self.m == "restore-no-plastic":
            data = data[:-2]
        assert len(items) == len(data)
        for (h, k), saved in zip(items, data):
            self._get(h, k)[:] = saved                                              # :443-446
        self.pcur = ck["pcur"]                                                      # :449
        self.substeps_done = ck["substeps_done"]                                    # :451
        if self.m != "restore-no-cur":
            self.cur = ck["bcur"]                                                   # :453-455
