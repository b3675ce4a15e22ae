"""The TDA rule of include/clipfs.h ("TDA") in fp64 numpy, twice:

    TDARef        the sequential rule, one sample at a time, with lists per class.  It records the margin of every
                  comparison it decides and counts the events, so that a test can assert ON THE REFERENCE that a case is
                  well conditioned before an fp32 result is compared with it.
    two_phase     a pure-Python model of the batch algorithm of csrc/tda.hip: per-row statistics, a scan per class that
                  turns the queue updates into [born, evict) intervals, masked sums over (old slots + batch rows), and a
                  write-back of the survivors.  test_tda_cpu.py proves it equal to the sequential rule.

Both work on the state layout of the device: pos_keys [C, Sp, d], pos_ent [C, Sp] (+inf = empty), pos_seq [C, Sp] int64
(-1 = empty), the same for the negative cache plus neg_mask [C, Sn, C] uint8, and counter (an int).
"""
import numpy as np

DEFAULTS = dict(logit_scale=100.0, pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0,
                ent_lo=0.2, ent_hi=0.5, mask_lo=0.03, mask_hi=1.0)
EVENTS = ("pos_free", "pos_evict", "pos_reject", "neg_free", "neg_evict", "neg_reject", "band_miss")
# the condition of the GPU tests: least margin of every decided comparison, by kind
MIN_MARGIN = dict(ent=1e-3, band=1e-3, mask=1e-4, top1=1e-2)


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def clustered(C, B, d, seed):
    """(T [C, d], F [B, d], y [B]): unit class and sample features whose cosines sit in a narrow band, as CLIP's do:
    T_c = unit(u + 0.35 g_c), f = unit(u + 1.05 a g_y + 0.35 n), a ~ U(0, 0.25), g, n ~ N(0, I / d), u a unit vector."""
    rng = np.random.default_rng(seed)
    u = unit(rng.standard_normal(d))
    g = rng.standard_normal((C, d)) / np.sqrt(d)
    y = rng.integers(0, C, B)
    a = rng.uniform(0.0, 0.25, B)
    n = rng.standard_normal((B, d)) / np.sqrt(d)
    T = unit(u + 0.35 * g)
    F = unit(u + 1.05 * a[:, None] * g[y] + 0.35 * n)
    # what the device gets is fp32: the reference works on exactly those numbers
    return T.astype(np.float32).astype(np.float64), F.astype(np.float32).astype(np.float64), y


def empty_state(C, d, Sp, Sn):
    return dict(pos_keys=np.zeros((C, Sp, d)), pos_ent=np.full((C, Sp), np.inf), pos_seq=np.full((C, Sp), -1, np.int64),
                neg_keys=np.zeros((C, Sn, d)), neg_ent=np.full((C, Sn), np.inf), neg_seq=np.full((C, Sn), -1, np.int64),
                neg_mask=np.zeros((C, Sn, C), np.uint8), counter=0)


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def stats(T, f, hp):
    """Steps 1 to 6 and the mask of step 8 for one sample: z, H, pred, h, in-band, m, p."""
    C = T.shape[0]
    z = hp["logit_scale"] * (T @ f)
    mx = z.max()
    lse = mx + np.log(np.exp(z - mx).sum())
    p = np.exp(z - lse)
    H = float(-(p * (z - lse)).sum())
    pred = int(np.argmax(z))  # the first maximum: ties to the lower index
    h = H / np.log2(C) if C > 1 else 0.0
    band = hp["ent_lo"] < h < hp["ent_hi"]
    m = ((hp["mask_lo"] < p) & (p < hp["mask_hi"])).astype(np.uint8)
    return z, H, pred, h, band, m, p


def _victim(queue):
    """The occupied slot of largest stored entropy, ties to the most recently inserted."""
    w = 0
    for k in range(1, len(queue)):
        if queue[k]["ent"] > queue[w]["ent"] or (queue[k]["ent"] == queue[w]["ent"] and queue[k]["seq"] > queue[w]["seq"]):
            w = k
    return w


class TDARef:
    """The sequential rule.  ``margins[kind]`` lists the margin of every decided comparison, ``events[name]`` counts."""

    def __init__(self, T, state=None, **hyper):
        self.T = np.asarray(T, np.float64)
        self.hp = {**DEFAULTS, **hyper}
        self.C, self.d = self.T.shape
        self.Sp, self.Sn = self.hp["pos_cap"], self.hp["neg_cap"]
        self.margins = {k: [] for k in MIN_MARGIN}
        self.events = {k: 0 for k in EVENTS}
        self.load(state if state is not None else empty_state(self.C, self.d, self.Sp, self.Sn))

    def load(self, st):
        self.t = int(st["counter"])
        self.pos = [[None] * self.Sp for _ in range(self.C)]  # per class: a list of slots, None = empty
        self.neg = [[None] * self.Sn for _ in range(self.C)]
        for c in range(self.C):
            for k in range(self.Sp):
                if st["pos_seq"][c, k] >= 0:
                    self.pos[c][k] = dict(key=st["pos_keys"][c, k].astype(np.float64), ent=float(st["pos_ent"][c, k]),
                                          seq=int(st["pos_seq"][c, k]))
            for k in range(self.Sn):
                if st["neg_seq"][c, k] >= 0:
                    self.neg[c][k] = dict(key=st["neg_keys"][c, k].astype(np.float64), ent=float(st["neg_ent"][c, k]),
                                          seq=int(st["neg_seq"][c, k]), mask=st["neg_mask"][c, k].copy())

    def state(self):
        st = empty_state(self.C, self.d, self.Sp, self.Sn)
        st["counter"] = self.t
        for name, queues in (("pos", self.pos), ("neg", self.neg)):
            for c, q in enumerate(queues):
                for k, e in enumerate(q):
                    if e is not None:
                        st[name + "_keys"][c, k], st[name + "_ent"][c, k], st[name + "_seq"][c, k] = e["key"], e["ent"], e["seq"]
                        if name == "neg":
                            st["neg_mask"][c, k] = e["mask"]
        return st

    def _offer(self, queue, entry, name):
        """Step 7 on one queue; returns the slot or -1."""
        if not queue:
            return -1
        free = [k for k, e in enumerate(queue) if e is None]
        if free:
            queue[free[0]] = entry
            self.events[name + "_free"] += 1
            return free[0]
        w = _victim(queue)
        self.margins["ent"].append(abs(entry["ent"] - queue[w]["ent"]))
        if np.float32(entry["ent"]) < np.float32(queue[w]["ent"]):
            queue[w] = entry
            self.events[name + "_evict"] += 1
            return w
        self.events[name + "_reject"] += 1
        return -1

    def logits(self, f, z):
        out = z.copy()
        hp = self.hp
        for c, q in enumerate(self.pos):
            for e in q:
                if e is not None:
                    out[c] += hp["pos_alpha"] * np.exp(-hp["pos_beta"] * (1.0 - f @ e["key"]))
        for q in self.neg:
            for e in q:
                if e is not None:
                    out -= hp["neg_alpha"] * np.exp(-hp["neg_beta"] * (1.0 - f @ e["key"])) * e["mask"]
        return out

    def step(self, f, update=True):
        """One sample: returns (out [C], record dict)."""
        hp = self.hp
        z, H, pred, h, band, m, p = stats(self.T, f, hp)
        ps = ns = -1
        if update:
            if self.C > 1:
                top = np.sort(z)
                self.margins["top1"].append(top[-1] - top[-2])
            ps = self._offer(self.pos[pred], dict(key=f.copy(), ent=H, seq=self.t), "pos")
            if self.Sn > 0:
                self.margins["band"].append(min(abs(h - hp["ent_lo"]), abs(h - hp["ent_hi"])))
                if band:
                    self.margins["mask"].append(min(np.abs(p - hp["mask_lo"]).min(), np.abs(p - hp["mask_hi"]).min()))
                    ns = self._offer(self.neg[pred], dict(key=f.copy(), ent=H, seq=self.t, mask=m), "neg")
                else:
                    self.events["band_miss"] += 1
            self.t += 1
        return self.logits(f, z), dict(pred=pred, entropy=H, hnorm=h, band=int(band), mask=m, pos_slot=ps, neg_slot=ns, z=z)

    def adapt(self, F, update=True):
        """B applications of ``step`` in row order: (out [B, C], record of stacked arrays)."""
        outs, recs = zip(*(self.step(f, update) for f in F))
        return np.stack(outs), {k: np.array([r[k] for r in recs]) for k in recs[0]}

    def well_conditioned(self, min_pos_evict=3, min_pos_reject=3):
        """The condition of the GPU tests, as a list of what fails (empty: the case qualifies)."""
        bad = [f"margin {k}: {min(v):.3g} < {MIN_MARGIN[k]}" for k, v in self.margins.items() if v and min(v) < MIN_MARGIN[k]]
        bad += [f"event {k} never occurs" for k, n in self.events.items() if n < 1]
        if self.events["pos_evict"] < min_pos_evict or self.events["pos_reject"] < min_pos_reject:
            bad.append(f"pos_evict {self.events['pos_evict']} / pos_reject {self.events['pos_reject']} below "
                       f"{min_pos_evict} / {min_pos_reject}")
        return bad


# ------------------------------------------------------------------------------------------------ the batch algorithm
def _scan(pred, H, take, ent, seq, B, t0, update):
    """One cache: per class a walk over the batch rows in order.  ``take[b]``: row b is offered to the queue of pred[b].
    Returns born, evict [C S + B], slot [B]; entry c S + k = old slot (c, k), entry C S + b = batch row b."""
    C, S = ent.shape
    born, evict = np.full(C * S + B, -7, np.int64), np.full(C * S + B, -7, np.int64)  # -7: not yet written
    slot = np.full(B, -1, np.int64)
    for b in range(B):  # rows that are not offered, and the rejected ones below: the empty interval
        if not (update and S > 0 and take[b]):
            born[C * S + b] = evict[C * S + b] = 0
    for c in range(C):  # one thread per class on the device
        q = [dict(ent=float(ent[c, k]), seq=int(seq[c, k]), owner=c * S + k, born=0) for k in range(S)]
        for e in q:  # an empty old slot is never in the cache; a batch row that takes the slot takes over its owner
            if e["seq"] < 0:
                born[e["owner"]] = evict[e["owner"]] = 0
        for b in range(B):
            if pred[b] != c or not (update and S > 0 and take[b]):
                continue
            free = [k for k in range(S) if q[k]["seq"] < 0]
            k = free[0] if free else -1
            if k < 0:
                w = _victim(q)
                if np.float32(H[b]) < np.float32(q[w]["ent"]):
                    k = w
                    born[q[w]["owner"]], evict[q[w]["owner"]] = q[w]["born"], b  # row b no longer sees the loser
            if k >= 0:
                q[k] = dict(ent=float(H[b]), seq=t0 + b, owner=C * S + b, born=b)
                slot[b] = k
            else:
                born[C * S + b] = evict[C * S + b] = 0
        for e in q:
            if e["seq"] >= 0:
                born[e["owner"]], evict[e["owner"]] = e["born"], B
    assert (born >= 0).all() and (evict >= 0).all(), "an interval was left unwritten"
    return born, evict, slot


def two_phase(T, F, state, update=True, **hyper):
    """The batch algorithm.  Returns (out [B, C], record, new state); ``state`` is not modified."""
    hp = {**DEFAULTS, **hyper}
    T, F = np.asarray(T, np.float64), np.asarray(F, np.float64)
    (C, d), B = T.shape, F.shape[0]
    Sp, Sn = hp["pos_cap"], hp["neg_cap"]
    t0 = int(state["counter"])
    # statistics: parallel over rows
    rows = [stats(T, f, hp) for f in F]
    z = np.stack([r[0] for r in rows])
    H = np.array([r[1] for r in rows])
    pred = np.array([r[2] for r in rows])
    hn = np.array([r[3] for r in rows])
    band = np.array([r[4] for r in rows])
    mask = np.stack([r[5] for r in rows])
    # scan
    pb, pe, pslot = _scan(pred, H, np.ones(B, bool), state["pos_ent"], state["pos_seq"], B, t0, update)
    nb, ne, nslot = _scan(pred, H, band, state["neg_ent"], state["neg_seq"], B, t0, update)
    # logits: entries = old slots then batch rows; entry j contributes to row i iff born_j <= i < evict_j
    i = np.arange(B)[:, None]
    out = z.copy()
    if Sp > 0:
        keys = np.concatenate([state["pos_keys"].reshape(C * Sp, d), F])
        cls = np.concatenate([np.repeat(np.arange(C), Sp), pred])
        G = hp["pos_alpha"] * np.exp(-hp["pos_beta"] * (1.0 - F @ keys.T)) * ((pb[None] <= i) & (i < pe[None]))
        out += G @ np.eye(C)[cls]
    if Sn > 0:
        keys = np.concatenate([state["neg_keys"].reshape(C * Sn, d), F])
        vals = np.concatenate([state["neg_mask"].reshape(C * Sn, C), mask]).astype(np.float64)
        G = hp["neg_alpha"] * np.exp(-hp["neg_beta"] * (1.0 - F @ keys.T)) * ((nb[None] <= i) & (i < ne[None]))
        out -= G @ vals
    # write-back: the survivors
    new = copy_state(state)
    if update:
        for b in range(B):
            if pslot[b] >= 0 and pe[C * Sp + b] == B:
                at = (pred[b], pslot[b])
                new["pos_keys"][at], new["pos_ent"][at], new["pos_seq"][at] = F[b], H[b], t0 + b
            if nslot[b] >= 0 and ne[C * Sn + b] == B:
                at = (pred[b], nslot[b])
                new["neg_keys"][at], new["neg_ent"][at], new["neg_seq"][at], new["neg_mask"][at] = F[b], H[b], t0 + b, mask[b]
        new["counter"] = t0 + B
    rec = dict(pred=pred, entropy=H, hnorm=hn, band=band.astype(np.int64), mask=mask, pos_slot=pslot, neg_slot=nslot,
               pos_born=pb, pos_evict=pe, neg_born=nb, neg_evict=ne, z=z)
    return out, rec, new


def state_equal(a, b):
    """Exact equality of two states (every array and the counter)."""
    return all(np.array_equal(a[k], b[k]) for k in a)
