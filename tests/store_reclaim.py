"""The store and the model of tests/store_gpu.py and tests/store_model.py with
the step that gives memory back, and the history tests/test_gpu_store_reclaim.py
runs. TEST INFRASTRUCTURE ONLY. Both classes subclass; nothing imported is
changed.

  ReclaimStore.reclaim()  one honu_key_reclaim over the store's whole device
                          state, one host read of the kept count and the byte
                          total, then n, the column (its first kept rows), the
                          order, keys, statuses, info, arena, sizes and offsets
                          are the call's outputs.
  ReclaimModel.reclaim()  the records become those of sorted(live), live
                          becomes all of them, the tail becomes empty.
"""
import numpy as np
import torch

import store_model as sm
from store_gpu import Store


class ReclaimStore(Store):
    def reclaim(self):
        """Returns (kept, bytes), read on the host once."""
        c, n = self.c, self.n
        R = c.reclaim_records(self.order, self.valid, n, self.arena, self.rec_off, n, self.rec_bytes,
                              max(self.rec_bytes, 16), keys=self.keys, key_status=self.key_status, info=self.info)
        # the one host read: the records that stay, for the next merge's b_base, and their bytes
        kept, total = torch.cat([R.kept, R.val_total]).cpu().tolist()
        sizes = (R.rec_off[1:kept + 1] - R.rec_off[:kept]).contiguous().view(torch.uint8)
        self.col, self.order = self.col[:29 * kept], R.order[:kept]  # valid stands: every valid row names its own record
        self.n, self.rec_bytes, self.removed = kept, total, None
        self.rec_off = R.rec_off[:kept + 1]
        # the growing buffers start again from the call's outputs, which have room for the records freed
        self._room_of = {"keys": (R.keys, 29 * kept), "key_status": (R.key_status.view(torch.uint8), 4 * kept),
                         "info": (R.info, 32 * kept), "arena": (R.values, total), "rec_size": (sizes, 8 * kept)}
        self.keys, self.key_status = R.keys[:29 * kept], R.key_status[:kept]
        self.info, self.arena, self.rec_size = R.info[:32 * kept], R.values[:total], sizes
        return kept, total


class ReclaimModel(sm.StoreModel):
    def __init__(self, marshal):
        super().__init__(marshal)
        self.batch = 0      # the batch that is being appended: the test counts it up
        self.batch_of = []  # per record, the batch that brought it

    def _append(self, key, rec, keybytes):
        super()._append(key, rec, keybytes)
        self.batch_of.append(self.batch)

    def live_bytes(self):
        return sum(len(self.records[i][2]) for i in self.live)

    def reclaim(self):
        """Returns what the coverage conditions ask about: the freed records' old indices, the batches that
        brought them, and how many of them carry a key that is byte-equal to a live row's."""
        keep = sorted(self.live)
        freed = [i for i in range(self.n) if i not in self.live]
        have = set(self.keys())
        out = dict(freed=freed, batches={self.batch_of[i] for i in freed},
                   equal=sum(1 for i in freed if self.keybytes[i] is not None and self.keybytes[i] in have),
                   source=keep)
        self.records = [self.records[i] for i in keep]
        self.keybytes = [self.keybytes[i] for i in keep]
        self.batch_of = [self.batch_of[i] for i in keep]
        self.live, self.tail, self._col = set(range(len(keep))), [], None
        return out


class History:
    """Two writes of about 1500, a drop of a third of the objects, a reclaim;
    Updates and Creates, Puts of stored keys, their compaction, a reclaim; a
    batch of tombstones, a reclaim with nothing to free. Then `peer`, what a
    second store writes, drops and reclaims before the first ships to it."""

    def __init__(self):
        rng = np.random.default_rng(6060)
        o = self.objs = sm._oids(rng, 1400, 0x10, 0xE0)
        self.absent = sm._oids(rng, 40, 0x10, 0xE0)
        self.new = sm._oids(rng, 100, 0xE0, 0xFF)
        self.dropped = o[0::3]                      # a third of the objects
        stay = np.concatenate([o[1::3], o[2::3]])
        pick = lambda pool, k: pool[rng.integers(0, len(pool), k)]  # noqa: E731
        W = lambda name, op, oids, seed, bad=0, skipped=0, pid=sm.PID: dict(  # noqa: E731
            name=name, kind="write", op=op, seed=seed, pid=pid, requests=sm._spoiled(oids, seed, bad, skipped))
        R = lambda name: dict(name=name, kind="reclaim")  # noqa: E731
        self.steps = [
            W("01 create", sm.CREATE, np.concatenate([o, pick(o, 60)]), 211, bad=20, skipped=20),
            W("02 update", sm.UPDATE, np.concatenate([o[:1300], pick(o, 150), self.absent]), 221, bad=5, skipped=5),
            dict(name="03 drop", kind="drop", prefixes=sm.request_rows(np.concatenate([self.dropped, self.dropped[:3]]), 231)),
            R("04 reclaim"),
            W("05 update", sm.UPDATE, np.concatenate([stay[:400], pick(stay, 40), self.dropped[:10]]), 241, bad=3, skipped=3),
            W("06 create", sm.CREATE, np.concatenate([self.new, self.dropped[20:70], stay[:10]]), 251),
            dict(name="07 put", kind="put_stored", count=50, seed=261),
            dict(name="08 compact", kind="compact"),
            R("09 reclaim"),
            W("10 delete", sm.DELETE, stay[500:620], 271),  # live objects, each once: every request is assigned
            R("11 reclaim"),
        ]
        self.peer = [
            W("p1 create", sm.CREATE, np.concatenate([o[:700], self.absent[:20]]), 311, bad=4, skipped=4),
            W("p2 update", sm.UPDATE, o[:300], 321, pid=9),
            dict(name="p3 drop", kind="drop", prefixes=sm.request_rows(o[0:700:5], 331)),
            R("p4 reclaim"),
        ]
        self.probes = sm.request_rows(np.concatenate([o, self.absent, self.new, np.zeros((1, 16), np.uint8)]), 97)


def apply_step(model: ReclaimModel, step, gen):
    """One step on the model: what store_model.apply_step returns, or ReclaimModel.reclaim's record."""
    if step["kind"] == "reclaim":
        return model.reclaim()
    model.batch += 1
    return sm.apply_step(model, step, gen)
