"""`bio::pattern_matching::myers::long::Myers<T>` (the block-based variant, DistType = usize) restated in Python integers,
line by line, as the definition the device kernels (csrc/myers_long.hip) and the mirror (rust_bio_amd/myers.py: MyersLong)
are compared with.  The word size `w` is a parameter: 8 is what the reference's own tests run (long.rs:594), 64 what the
device implements.  No `u128`, no lazy interface.

`band`: the max_dist the Ukkonen band is run with (States::new / States::step); None means the search's own max_dist, as in
the reference.  band >= m keeps every block in every column (long.rs:206, 263): the tests compare the two, which is what
lets the device compute all blocks.

The plain DP, the path check, the record helpers and the trim rule are those of tests/myers_oracle.py."""
import numpy as np

from myers_oracle import (ALN_DTYPE, DEL, INS, MATCH, MIN_SCORE, SUBST, check_path, dp_columns, hit_record,  # noqa: F401
                          no_hit_record, trim_range, TRIM_3P, TRIM_5P)

USIZE = (1 << 64) - 1  # usize::MAX


def ceil_div(a, b):
    return (a + b - 1) // b


class State:  # myers_impl.rs:10-18 with D = usize
    __slots__ = ("pv", "mv", "dist")

    def __init__(self, pv=0, mv=0, dist=0):  # Default: all zero
        self.pv, self.mv, self.dist = pv, mv, dist

    def copy(self):
        return State(self.pv, self.mv, self.dist)

    def adjust_up_by(self, range_mask):  # myers_impl.rs:70-77
        p = bin(self.pv & range_mask).count("1")
        m = bin(self.mv & range_mask).count("1")
        self.dist = (self.dist + m - p) & USIZE

    def adjust_one_up(self, pos_mask):  # myers_impl.rs:97-103
        if self.pv & pos_mask:
            self.dist = (self.dist - 1) & USIZE
        elif self.mv & pos_mask:
            self.dist = (self.dist + 1) & USIZE


class Peq:  # long.rs:32-44
    __slots__ = ("peq", "high_mask")

    def __init__(self, peq, high_mask):
        self.peq, self.high_mask = peq, high_mask


def build_peq(pattern, ambigs, wildcards, w):
    """new_ambig, long.rs:70-122: ([Peq], m)"""
    pattern = bytes(pattern)
    m = len(pattern)
    if m == 0:
        raise ValueError("Pattern is empty")  # long.rs:83
    W = (1 << w) - 1
    peq = []
    for c0 in range(0, m, w):  # long.rs:88
        block = [0] * 256
        chunk_len = 0
        for symbol in pattern[c0:c0 + w]:
            mask = 1 << chunk_len
            block[symbol] |= mask
            if ambigs and symbol in ambigs:
                for eq in ambigs[symbol]:
                    block[eq] |= mask
            chunk_len += 1
        for wc in wildcards or ():  # long.rs:105-109
            block[wc] = W
        peq.append(Peq(block, 1 << (chunk_len - 1)))  # long.rs:111-114
    return peq, m


def advance_block(state, p, a, hin, W):  # long.rs:136-179
    eq = p.peq[a]
    xv = eq | state.mv
    if hin < 0:
        eq |= 1
    xh = ((((eq & state.pv) + state.pv) & W) ^ state.pv) | eq  # wrapping_add
    ph = state.mv | (~(xh | state.pv) & W)
    mh = state.pv & xh
    hout = (1 if ph & p.high_mask else 0) - (1 if mh & p.high_mask else 0)
    state.dist = (state.dist + hout) & USIZE
    ph = (ph << 1) & W
    mh = (mh << 1) & W
    if hin < 0:
        mh |= 1
    if hin > 0:
        ph |= 1
    state.pv = mh | (~(xv | ph) & W)
    state.mv = ph & xv
    return hout


class States:  # long.rs:183-275
    def __init__(self, m, max_dist, w):  # new, long.rs:196-211
        self.w, self.W = w, (1 << w) - 1
        nblock = ceil_div(m, w)
        self.states = []
        self.max_block_i = nblock - 1
        self.last_m = m % w
        min_blocks = max(1, ceil_div(min(max_dist, m), w))  # long.rs:206
        for _ in range(min_blocks):
            self.add_block(0)

    def add_block(self, carry):  # long.rs:216-236
        prev_dist = self.states[-1].dist if self.states else 0
        if len(self.states) == self.max_block_i and self.last_m > 0:
            delta = self.last_m
        else:
            delta = self.w
        self.states.append(State(self.W, 0, (prev_dist + delta + carry) & USIZE))  # State::init

    def step(self, a, peq, max_dist):  # long.rs:239-268
        carry = 0
        y = len(self.states) - 1
        for state, block_peq in zip(self.states, peq):
            carry = advance_block(state, block_peq, a, carry, self.W)
        last_dist = self.states[y].dist
        if (((last_dist - carry) & USIZE) <= max_dist and y < self.max_block_i
                and (peq[y + 1].peq[a] & 1 == 1 or carry < 0)):  # long.rs:253-256
            y += 1
            self.add_block(-carry)
            advance_block(self.states[y], peq[y], a, carry, self.W)
        else:
            while y > 0 and self.states[y].dist >= max_dist + self.w:  # long.rs:263
                y -= 1
            del self.states[y + 1:]

    def known_dist(self):  # long.rs:272-274
        return self.states[self.max_block_i].dist if self.max_block_i < len(self.states) else None


class Traceback:
    """traceback.rs:130-318 with LongStatesHandler (long.rs:295-372)"""

    def __init__(self, initial, num_cols, m, w):  # traceback.rs:153-186
        num_cols += 2  # two additional columns at the left of the matrix
        self.m, self.w, self.W, self.num_cols = m, w, (1 << w) - 1, num_cols
        self.n_blocks = ceil_div(m, w)  # init, long.rs:303-307
        self.states = [State() for _ in range(num_cols * self.n_blocks)]  # resize_with(Default)
        self._next = 0
        self.pos = self._advance()
        for i in range(self.n_blocks):  # set_max_state, long.rs:315-320
            self.states[self.pos * self.n_blocks + i] = State(self.W, 0, USIZE)
        self.add_state(initial)

    def _advance(self):  # positions: (0..num_cols).cycle()
        p = self._next
        self._next = (self._next + 1) % self.num_cols
        return p

    def add_state(self, column):  # traceback.rs:189-192, long.rs:323-350
        self.pos = self._advance()
        source = column.states
        pos = self.pos * self.n_blocks
        for i, s in enumerate(source):
            self.states[pos + i] = s.copy()
        if len(source) < self.n_blocks:
            self.states[pos + len(source)] = State(0, 0, USIZE)  # the "barrier"
            self.states[pos + self.n_blocks - 1].dist = USIZE  # the marker of a column that is not complete

    def _columns(self, pos):  # long.rs:415-419: states[..n_blocks * (pos + 1)].chunks().rev().chain(chunks().rev().cycle())
        nb = self.n_blocks
        for c in range(pos, -1, -1):
            yield self.states[c * nb:(c + 1) * nb]
        while True:
            for c in range(self.num_cols - 1, -1, -1):
                yield self.states[c * nb:(c + 1) * nb]

    def traceback(self):
        """_traceback_at(self.pos), traceback.rs:235-318, with LongTracebackHandler (long.rs:402-563): (length, dist, ops in
        reverse) or None"""
        w, W, n_blocks = self.w, self.W, self.n_blocks
        # LongTracebackHandler::new, long.rs:404-453
        last_m = self.m % w
        if last_m == 0:
            last_m = w
        mask0 = 1 << (last_m - 1)
        it = self._columns(self.pos)
        col = next(it)
        left_col = next(it)
        if col[-1].dist == USIZE:  # long.rs:425
            return None
        if last_m == 1 and n_blocks > 1:  # long.rs:430-434
            left_block_idx, left_adj_mask, max_mask = n_blocks - 2, 0, 1 << (w - 1)
        else:
            left_block_idx, left_adj_mask, max_mask = n_blocks - 1, mask0, mask0
        left_block = left_col[left_block_idx].copy()
        left_block.adjust_up_by(left_adj_mask)
        block = col[n_blocks - 1].copy()
        block_idx = n_blocks - 1
        pos_mask = mask0

        h_offset, dist, ops = 0, block.dist, []
        while not (pos_mask == 0 and block_idx == 0):  # done(), long.rs:561-563
            move_left = True
            diagonal = False
            if (left_block.dist + 1) & USIZE == block.dist:  # Subst, traceback.rs:265-270
                diagonal, op = True, SUBST
            elif block.pv & pos_mask:  # try_move_up + move_up, long.rs:488-517: Ins
                if pos_mask != 1 or block_idx == 0:
                    block.adjust_one_up(pos_mask)
                    pos_mask >>= 1
                else:
                    pos_mask = 1 << (w - 1)
                    block_idx -= 1
                    block = col[block_idx].copy()
                # adjust_left_up, long.rs:461-473
                at_boundary = bool(left_adj_mask & 0b10) and left_block_idx > 0
                if not at_boundary:
                    left_adj_mask = (left_adj_mask >> 1) | max_mask
                    left_block.adjust_one_up(pos_mask)
                else:
                    max_mask = 1 << (w - 1)
                    left_adj_mask = 0
                    left_block_idx -= 1
                    left_block = left_col[left_block_idx].copy()
                op, move_left = INS, False
            else:  # try_prepare_left, long.rs:532-550: Del
                is_del = False
                if left_adj_mask != 0:
                    if left_block.mv & pos_mask:
                        left_block.dist = (left_block.dist - 1) & USIZE
                        is_del = True
                elif left_block_idx + 1 < len(left_col):
                    b = left_col[left_block_idx + 1]
                    if b.mv & 1 == 1:
                        d = (left_block.dist - 1) & USIZE
                        left_block = b.copy()
                        left_block.dist = d
                        is_del = True
                if is_del:
                    op = DEL
                else:  # Match, traceback.rs:281-284
                    diagonal, op = True, MATCH
            if diagonal:  # prepare_diagonal, long.rs:520-530
                at_boundary = bool(left_adj_mask & 0b10) and left_block_idx > 0
                if not at_boundary:
                    left_adj_mask = (left_adj_mask >> 1) | max_mask
                else:
                    max_mask = 1 << (w - 1)
                    left_adj_mask = 0
                    left_block_idx -= 1
                if pos_mask != 1 or block_idx == 0:
                    pos_mask >>= 1
                else:
                    pos_mask = 1 << (w - 1)
                    block_idx -= 1
            if move_left:  # traceback.rs:305-306; finish_move_left, long.rs:553-558
                h_offset += 1
                col = left_col
                left_col = next(it)
                block = left_block
                left_block = left_col[left_block_idx].copy()
                left_block.adjust_up_by(left_adj_mask)
            ops.append(op)
        return h_offset, dist, ops


class MyersLong:
    def __init__(self, pattern, ambigs=None, wildcards=None, w=64):
        self.w = w
        self.peq, self.m = build_peq(pattern, ambigs, wildcards, w)
        self.max_dist_limit = USIZE - w  # impl_myers!'s $max_dist, long.rs:586
        self._memo = {}

    def full_peq(self):
        """the blocks' tables as one integer per byte (bit i: pattern symbol i matches), for the plain DP"""
        out = [0] * 256
        for b, p in enumerate(self.peq):
            chunk = (p.high_mask << 1) - 1
            for a in range(256):
                out[a] |= (p.peq[a] & chunk) << (b * self.w)
        return out

    def distance(self, text):  # myers_impl.rs:163-181
        max_dist = self.max_dist_limit
        dist = max_dist
        st = States(self.m, max_dist, self.w)
        for a in bytes(text):
            st.step(a, self.peq, max_dist)
            d = st.known_dist()
            if d is not None and d < dist:
                dist = d
        return dist

    def find_all_end(self, text, max_dist, band=None):  # myers_impl.rs:185-195, 264-294
        max_dist = min(max_dist, self.max_dist_limit)
        band = max_dist if band is None else band
        st = States(self.m, band, self.w)
        out = []
        for i, a in enumerate(bytes(text)):
            st.step(a, self.peq, band)
            d = st.known_dist()
            if d is not None and d <= max_dist:
                out.append((i, d))
        return out

    def find_best_end(self, text):  # myers_impl.rs:199-207
        hits = self.find_all_end(text, self.max_dist_limit)
        if not hits:
            raise ValueError("find_best_end of an empty text")
        return min(hits, key=lambda h: h[1])

    def find_all(self, text, max_dist, band=None):
        """FullMatches (myers_impl.rs:323-346, 352-369, 456-494) with next_alignment at every hit: a list of
        (start, end + 1, dist, ops in pattern order)"""
        text = bytes(text)
        max_dist = min(max_dist, self.max_dist_limit)
        key = (text, max_dist, band)
        if key not in self._memo:
            self._memo[key] = self._find_all(text, max_dist, max_dist if band is None else band)
        return self._memo[key]

    def _find_all(self, text, max_dist, band):
        st = States(self.m, band, self.w)
        num_cols = self.m + min(max_dist, self.m)  # myers_impl.rs:327
        tb = Traceback(st, num_cols, self.m, self.w)
        out = []
        for i, a in enumerate(text):
            st.step(a, self.peq, band)  # step_trace, myers_impl.rs:151-160
            tb.add_state(st)
            d = st.known_dist()
            if d is not None and d <= max_dist:
                length, dist, ops = tb.traceback()  # .unwrap()
                assert dist == d
                out.append((i + 1 - length, i + 1, dist, ops[::-1]))
        return out


# ---- the records of the batch calls (the conventions of myers_oracle.best_records / find_all_records) ------------------
def best_hit(my, text, max_dist):
    hits = my.find_all(text, max_dist)
    return min(hits, key=lambda h: h[2]) if hits else None


def best_records(myers_list, texts, max_dist, ops_stride=None):
    """bg_myers_long_best_batch: records of job t * n_pat + p and, with ops_stride, the strided operation buffer"""
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
    """bg_myers_long_find_all_batch: (records[n_jobs * max_hits], count[n_jobs])"""
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
