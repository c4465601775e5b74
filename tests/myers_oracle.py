"""`bio::pattern_matching::myers::Myers<u64>` restated in Python integers masked to 64 bits, line by line, as the
definition the device kernels (csrc/myers.hip) and the mirror (rust_bio_amd/myers.py) are compared with.  Only the
`u64` flavour (patterns of 1 to 64 symbols, DistType = u8); no `myers::long`, no `u128`, no lazy interface.

Also here: a plain O(mn) semiglobal edit-distance DP and a path-consistency check (the restatement's own test), the
records a batch call must return (`best_records`, `find_all_records`) and the trim rule of bg_fastq_trim[_dev]
(`trim_range`), which the reference does not have and include/biogpu.h defines."""
import numpy as np

M64 = (1 << 64) - 1
MATCH, SUBST, DEL, INS = 0, 1, 2, 3  # BG_OP_*: Ins consumes a pattern symbol (x), Del a text byte (y)
MIN_SCORE = -858993459
MODE_SEMIGLOBAL = 2
ALN_DTYPE = np.dtype([("score", "<i4"), ("xstart", "<u4"), ("xend", "<u4"), ("ystart", "<u4"), ("yend", "<u4"), ("xlen", "<u4"),
                      ("ylen", "<u4"), ("n_ops", "<u4"), ("ops_off", "<u8"), ("clip_len", "<u4", (4,)), ("n_clips", "u1"),
                      ("mode", "u1"), ("status", "i1"), ("_pad", "u1"), ("_tail", "<u4")])


class State:  # myers_impl.rs:10-18
    __slots__ = ("pv", "mv", "dist")

    def __init__(self, pv=0, mv=0, dist=0):  # Default: all zero
        self.pv, self.mv, self.dist = pv, mv, dist

    @staticmethod
    def init(m):  # myers_impl.rs:28-34
        return State(M64, 0, m)

    @staticmethod
    def init_max_dist():  # myers_impl.rs:38-40: D::max_value() of u8
        return State.init(255)

    def copy(self):
        return State(self.pv, self.mv, self.dist)

    def adjust_up_by(self, range_mask):  # myers_impl.rs:70-77
        p = bin(self.pv & range_mask).count("1")
        m = bin(self.mv & range_mask).count("1")
        self.dist = (self.dist + m - p) & 0xFF

    def adjust_one_up(self, pos_mask):  # myers_impl.rs:97-103
        if self.pv & pos_mask:
            self.dist = (self.dist - 1) & 0xFF
        elif self.mv & pos_mask:
            self.dist = (self.dist + 1) & 0xFF


def build_peq(pattern, ambigs=None, wildcards=None):
    """new_ambig, simple.rs:39-82: (peq[256], m).  Raises where the reference asserts."""
    m = len(pattern)
    if m > 64:
        raise ValueError("Pattern too long")  # simple.rs:52
    if m == 0:
        raise ValueError("Pattern is empty")  # simple.rs:53
    peq = [0] * 256  # simple.rs:55
    for i, symbol in enumerate(bytes(pattern)):  # simple.rs:57-68
        mask = 1 << i
        peq[symbol] |= mask
        if ambigs and symbol in ambigs:
            for eq in ambigs[symbol]:
                peq[eq] |= mask
    for w in wildcards or ():  # simple.rs:70-74
        peq[w] = M64
    return peq, m


class Myers:
    def __init__(self, pattern, ambigs=None, wildcards=None):
        self.peq, self.m = build_peq(pattern, ambigs, wildcards)
        self.bound = 1 << (self.m - 1)  # simple.rs:78
        self._memo = {}  # find_all answers by (text, max_dist): the tests ask the same question of several calls

    def step(self, st, a):  # _step, simple.rs:95-117
        eq = self.peq[a]
        xv = eq | st.mv
        xh = (((((eq & st.pv) + st.pv) & M64) ^ st.pv) | eq) & M64  # wrapping_add
        ph = (st.mv | (~(xh | st.pv) & M64)) & M64
        mh = st.pv & xh
        diff = (1 if ph & self.bound else 0) - (1 if mh & self.bound else 0)
        st.dist = (st.dist + diff) & 0xFF  # the u8 the reference converts back to
        ph = (ph << 1) & M64
        mh = (mh << 1) & M64
        st.pv = (mh | (~(xv | ph) & M64)) & M64
        st.mv = ph & xv

    def distance(self, text):  # myers_impl.rs:163-181
        dist = 255
        st = State.init(self.m)
        for a in bytes(text):
            self.step(st, a)
            if st.dist < dist:
                dist = st.dist
        return dist

    def find_all_end(self, text, max_dist):  # myers_impl.rs:185-195, 284-294
        max_dist = min(max_dist, 255)
        st = State.init(self.m)
        out = []
        for i, a in enumerate(bytes(text)):
            self.step(st, a)
            if st.dist <= max_dist:
                out.append((i, st.dist))
        return out

    def find_best_end(self, text):  # myers_impl.rs:199-207: min_by_key keeps the first of equals; unwrap panics on no hit
        hits = self.find_all_end(text, 255)
        if not hits:
            raise ValueError("find_best_end of an empty text")
        return min(hits, key=lambda h: h[1])

    def find_all(self, text, max_dist):
        """FullMatches (myers_impl.rs:323-346, 352-369, 456-494) with next_alignment at every hit: a list of
        (start, end + 1, dist, ops in pattern order)."""
        text = bytes(text)
        max_dist = min(max_dist, 255)
        if (text, max_dist) not in self._memo:
            self._memo[(text, max_dist)] = self._find_all(text, max_dist)
        return self._memo[(text, max_dist)]

    def _find_all(self, text, max_dist):
        st = State.init(self.m)
        num_cols = self.m + min(max_dist, self.m)  # myers_impl.rs:327
        tb = Traceback(st, num_cols, self.m)
        out = []
        for i, a in enumerate(text):
            self.step(st, a)  # step_trace, myers_impl.rs:151-160
            tb.add_state(st)
            if st.dist <= max_dist:
                length, dist, ops = tb.traceback()
                assert dist == st.dist
                out.append((i + 1 - length, i + 1, dist, ops[::-1]))
        return out


class Traceback:  # traceback.rs:130-318
    def __init__(self, initial_state, num_cols, m):  # traceback.rs:153-186
        num_cols += 2  # two additional columns at the left of the matrix
        self.m, self.num_cols = m, num_cols
        self.states = [State() for _ in range(num_cols)]
        self._next = 0
        self.pos = self._advance()  # first column: the max state (a text shorter than the pattern)
        self.states[self.pos] = State.init_max_dist()
        self.add_state(initial_state)

    def _advance(self):  # positions: (0..num_cols).cycle()
        p = self._next
        self._next = (self._next + 1) % self.num_cols
        return p

    def add_state(self, st):  # traceback.rs:189-192
        self.pos = self._advance()
        self.states[self.pos] = st.copy()

    def traceback(self):  # _traceback_at(self.pos), traceback.rs:235-318, with ShortTracebackHandler (simple.rs:202-297)
        states, m = self.states, self.m
        pos_mask = 1 << (m - 1)  # simple.rs:205
        it = _rev_chain_cycle(states, self.pos)  # simple.rs:211-214
        block = next(it).copy()
        left = next(it).copy()
        left.adjust_one_up(pos_mask)  # simple.rs:222
        max_mask, left_adj_mask = pos_mask, pos_mask
        h_offset, dist, ops = 0, block.dist, []
        while pos_mask:  # done(), simple.rs:299-301
            move_left = True
            if (left.dist + 1) & 0xFF == block.dist:  # Subst, traceback.rs:265-270
                left_adj_mask = (left_adj_mask >> 1) | max_mask  # prepare_diagonal, simple.rs:287-290
                pos_mask >>= 1
                op = SUBST
            elif block.pv & pos_mask:  # try_move_up, simple.rs:259-275: Ins
                block.adjust_one_up(pos_mask)
                pos_mask >>= 1
                left_adj_mask = (left_adj_mask >> 1) | max_mask
                left.adjust_one_up(pos_mask)
                op, move_left = INS, False
            elif left.mv & pos_mask:  # try_prepare_left, simple.rs:278-284: Del
                left.dist = (left.dist - 1) & 0xFF
                op = DEL
            else:  # Match, traceback.rs:281-284
                left_adj_mask = (left_adj_mask >> 1) | max_mask
                pos_mask >>= 1
                op = MATCH
            if move_left:  # traceback.rs:305-306, finish_move_left simple.rs:293-296
                h_offset += 1
                block = left
                left = next(it).copy()
                left.adjust_up_by(left_adj_mask)
            ops.append(op)
        return h_offset, dist, ops


def _rev_chain_cycle(states, pos):
    for i in range(pos, -1, -1):
        yield states[i]
    while True:
        for i in range(len(states) - 1, -1, -1):
            yield states[i]


# ---- the plain DP and the consistency check ---------------------------------------------------------------------------
def dp_columns(peq, m, text):
    """semiglobal edit distance by the textbook recurrence: D[i][-1] = i, D[0][j] = 0; returns D[m][j] for every j"""
    prev = list(range(m + 1))
    out = []
    for a in bytes(text):
        cur = [0] * (m + 1)
        for i in range(1, m + 1):
            cur[i] = min(prev[i - 1] + (0 if peq[a] >> (i - 1) & 1 else 1), prev[i] + 1, cur[i - 1] + 1)
        out.append(cur[m])
        prev = cur
    return out


def check_path(peq, m, text, start, end, dist, ops):
    """ops consume all m pattern symbols, run from `start` to `end` of the text, agree with the two strings and cost dist"""
    assert start >= 0
    i, j, cost = 0, start, 0
    for op in ops:
        if op in (MATCH, SUBST):
            assert (peq[text[j]] >> i & 1) == (1 if op == MATCH else 0), (i, j, op)
            cost += op == SUBST
            i, j = i + 1, j + 1
        elif op == INS:
            i, cost = i + 1, cost + 1
        else:
            assert op == DEL
            j, cost = j + 1, cost + 1
    assert (i, j, cost) == (m, end, dist), (i, j, cost, m, end, dist)


# ---- the records of the batch calls -----------------------------------------------------------------------------------
def no_hit_record(m, ylen):
    r = np.zeros((), dtype=ALN_DTYPE)
    r["score"], r["xlen"], r["ylen"], r["mode"] = MIN_SCORE, m, ylen, MODE_SEMIGLOBAL
    return r


def hit_record(m, ylen, start, end, dist, n_ops=0, ops_off=0):  # update_aln, helpers.rs:83-99
    r = np.zeros((), dtype=ALN_DTYPE)
    r["score"], r["xend"], r["xlen"], r["ylen"], r["yend"], r["ystart"] = dist, m, m, ylen, end, start
    r["mode"], r["n_ops"], r["ops_off"] = MODE_SEMIGLOBAL, n_ops, ops_off
    return r


def best_hit(my, text, max_dist):
    """find_all(text, max_dist).min_by_key(dist): (start, end + 1, dist, ops) or None"""
    hits = my.find_all(text, max_dist)
    return min(hits, key=lambda h: h[2]) if hits else None


def best_records(myers_list, texts, max_dist, ops_stride=None):
    """bg_myers_best_batch: records of job t * n_pat + p and, with ops_stride, the strided operation buffer (a job's
    operations end at the end of its slot)."""
    n_pat = len(myers_list)
    rec = np.zeros(len(texts) * n_pat, dtype=ALN_DTYPE)
    ops = np.zeros(len(rec) * (ops_stride or 0), dtype=np.uint8)
    for t, text in enumerate(texts):
        for p, my in enumerate(myers_list):
            j = t * n_pat + p
            h = best_hit(my, text, max_dist)
            if h is None:
                rec[j] = no_hit_record(my.m, len(text))
                continue
            start, end, dist, o = h
            if ops_stride is None:
                rec[j] = hit_record(my.m, len(text), start, end, dist, len(o), 0)
            else:
                assert len(o) <= ops_stride
                rec[j] = hit_record(my.m, len(text), start, end, dist, len(o), (j + 1) * ops_stride - len(o))
                ops[(j + 1) * ops_stride - len(o):(j + 1) * ops_stride] = o
    return rec, ops


def find_all_records(myers_list, texts, max_dist, max_hits, ends_only):
    """bg_myers_find_all_batch: (records[n_jobs * max_hits], count[n_jobs])"""
    n_pat = len(myers_list)
    rec = np.zeros(len(texts) * n_pat * max_hits, dtype=ALN_DTYPE)
    count = np.zeros(len(texts) * n_pat, dtype=np.uint32)
    for t, text in enumerate(texts):
        for p, my in enumerate(myers_list):
            j = t * n_pat + p
            if ends_only:
                hits = [(e + 1, e + 1, d) for e, d in my.find_all_end(text, max_dist)]
            else:
                hits = [h[:3] for h in my.find_all(text, max_dist)]
            count[j] = len(hits)
            for s in range(max_hits):
                rec[j * max_hits + s] = hit_record(my.m, len(text), *hits[s]) if s < len(hits) else no_hit_record(my.m, len(text))
    return rec, count


# ---- the trim rule (include/biogpu.h, bg_fastq_trim) ----------------------------------------------------------------
TRIM_3P, TRIM_5P = 0, 1


def trim_range(mode, hits, seq_len, qual_len):
    """hits: the read's (score, ystart, yend) per pattern.  Returns ((seq lo, seq hi), (qual lo, qual hi))."""
    lo, hi = 0, seq_len
    have = [(ys, ye) for sc, ys, ye in hits if sc != MIN_SCORE]
    if mode == TRIM_3P:
        if have:
            hi = min(seq_len, min(ys for ys, _ in have))
    else:
        if have:
            lo = min(seq_len, max(ye for _, ye in have))
    return (lo, hi), (min(lo, qual_len), min(hi, qual_len))
