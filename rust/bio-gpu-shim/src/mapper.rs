//! Seed-and-extend in one call (`bg_seed_extend_batch`): the composition rust-bio's callers write by hand from
//! `backward_search`, `Interval::occ` and `Aligner::semiglobal` (src/lib.rs:129-165, benches/fmindex.rs:20-38), on the
//! forward strand or on both (`bg_seed_extend_strands_batch`: the `dna::revcomp` of each read as well), or as read pairs
//! (`bg_seed_extend_pairs_batch`: interleaved mates, the best proper FR pair where there is one), or with runner-up loci and a
//! MAPQ per read (`bg_seed_extend_multi_batch`), or as read pairs with a MAPQ per mate (`bg_seed_extend_pairs_mapq_batch`; with mate
//! rescue as well: `bg_seed_extend_pairs_rescue_mapq_batch`).
use crate::fmindex::GpuFMIndex;
use crate::pairwise::{scoring_to_c, tabulate};
use crate::{concat, strerror, sys, to_alignment, zero_alignment};
use bio::alignment::pairwise::{MatchFunc, Scoring};
use bio_types::alignment::Alignment;

pub struct Hit {
    /// `Aligner::semiglobal(read, window)` of the best candidate; `None`: no seed voted
    pub alignment: Option<Alignment>,
    pub ref_start: usize,
    pub ref_end: usize,
    pub n_candidates: u32,
    /// the winner is on the reverse strand: `alignment` is of `dna::revcomp(read)` against the forward text (SAM's convention)
    pub reverse: bool,
}

pub struct PairHit {
    /// mate 1, mate 2
    pub mates: [Hit; 2],
    /// both mates report the chosen proper FR pair (SAM FLAG 0x2)
    pub proper: bool,
    /// of the proper pair (SAM |TLEN|); 0 when not proper
    pub span: u64,
    /// proper combinations among the pair's candidates, both orientations
    pub n_proper: u32,
    /// `seed_extend_batch_pairs_rescue`: 1 / 2 = the mate that was placed inside its partner's insert window, 0 otherwise
    pub rescued: u8,
}

/// `seed_extend_batch_pairs_mapq` / `seed_extend_batch_pairs_rescue_mapq`: how unique each mate's placement is, mate 1 and mate 2
pub struct PairQuality {
    /// judged against the pair where it is proper (0: another placement of the mate serves the pair as well; `mapq_cap`: the mate has
    /// no other placement), as `seed_extend_batch_multi` judges a single read where it is not
    pub mapq: [u8; 2],
    /// score of the mate's best alternative placement (runner-up locus); `BG_MIN_SCORE` if there is none
    pub sub_score: [i32; 2],
    /// 1, or 2 with an alternative; 0 for a mate without a placement of at least `min_score` in a pair that is not proper
    pub n_loci: [u32; 2],
}

pub struct MultiHit {
    /// the read's loci in rank order, the best first (empty: unmapped); their text intervals do not touch
    pub hits: Vec<Hit>,
    /// 0 where the runner-up scores as much as the best, `mapq_cap` where there is none
    pub mapq: u8,
    /// score of the runner-up locus; `BG_MIN_SCORE` if there is none
    pub sub_score: i32,
    /// loci found, counted up to max(max_hits, 2)
    pub n_loci: u32,
}

impl GpuFMIndex<'_> {
    /// the text the index was built from, final sentinel included (windows are cut from it)
    pub fn attach_text(&mut self, text: &[u8]) {
        let rc = unsafe { sys::bg_fm_set_text(self.h, text.as_ptr(), text.len() as u64) };
        assert!(rc == 0, "{}", strerror(rc));
    }

    pub fn seed_extend_batch<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], seed_len: u32, stride: u32,
                                           max_occ: u32, pad: u32) -> Vec<Hit> {
        let table = tabulate(scoring);
        let sc = scoring_to_c(scoring, &table);
        let prm = sys::bg_seed_params_t { seed_len, stride, max_occ, pad };
        let (buf, off) = concat(reads);
        let zero = sys::bg_seed_hit_t { aln: zero_alignment(), window_start: 0, ref_start: 0, ref_end: 0, n_candidates: 0, n_seed_hits: 0 };
        let mut hits = vec![zero; reads.len()];
        let mut ops = vec![0u8; 2 * buf.len() + (2 * pad as usize + 4) * reads.len() + 8];
        let mut used = 0u64;
        let rc = unsafe {
            sys::bg_seed_extend_batch(self.h, &sc, &prm, reads.len() as u64, buf.as_ptr(), off.as_ptr(), hits.as_mut_ptr(),
                                      ops.as_mut_ptr(), ops.len() as u64, &mut used)
        };
        assert!(rc == 0, "{}", strerror(rc));
        hits.iter()
            .map(|h| Hit {
                alignment: if h.aln.score == sys::BG_MIN_SCORE { None } else { Some(to_alignment(&h.aln, &ops)) },
                ref_start: h.ref_start as usize,
                ref_end: h.ref_end as usize,
                n_candidates: h.n_candidates,
                reverse: false,
            })
            .collect()
    }

    /// `strands`: `sys::BG_STRAND_FORWARD`, `_REVERSE` or `_BOTH` (as u32).  The reads go in as given; the library builds the reverse
    /// complements itself.  With both strands the higher score wins, the forward strand on an equal score.
    pub fn seed_extend_batch_strands<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], strands: u32, seed_len: u32,
                                                   stride: u32, max_occ: u32, pad: u32) -> Vec<Hit> {
        let table = tabulate(scoring);
        let sc = scoring_to_c(scoring, &table);
        let prm = sys::bg_seed_params_t { seed_len, stride, max_occ, pad };
        let (buf, off) = concat(reads);
        let zero = sys::bg_seed_hit_t { aln: zero_alignment(), window_start: 0, ref_start: 0, ref_end: 0, n_candidates: 0, n_seed_hits: 0 };
        let mut hits = vec![zero; reads.len()];
        let mut strand = vec![0u8; reads.len()];
        let mut ops = vec![0u8; 2 * buf.len() + (2 * pad as usize + 4) * reads.len() + 8];
        let mut used = 0u64;
        let rc = unsafe {
            sys::bg_seed_extend_strands_batch(self.h, &sc, &prm, strands, reads.len() as u64, buf.as_ptr(), off.as_ptr(),
                                              hits.as_mut_ptr(), strand.as_mut_ptr(), ops.as_mut_ptr(), ops.len() as u64, &mut used)
        };
        assert!(rc == 0, "{}", strerror(rc));
        hits.iter()
            .zip(strand.iter())
            .map(|(h, &s)| Hit {
                alignment: if h.aln.score == sys::BG_MIN_SCORE { None } else { Some(to_alignment(&h.aln, &ops)) },
                ref_start: h.ref_start as usize,
                ref_end: h.ref_end as usize,
                n_candidates: h.n_candidates,
                reverse: s as i32 == sys::BG_HIT_REVERSE,
            })
            .collect()
    }

    /// Read pairs: `reads[2p]`, `reads[2p + 1]` are the mates of pair p, each mapped on both strands.  Where the best proper FR
    /// combination (span in `min_span ..= max_span`) gives up at most `pen_unpaired` of score against the mates' own bests, both
    /// mates report it and the pair is proper; otherwise each mate reports what `seed_extend_batch_strands` reports for it.
    pub fn seed_extend_batch_pairs<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], min_span: u32, max_span: u32,
                                                 pen_unpaired: i32, seed_len: u32, stride: u32, max_occ: u32, pad: u32)
                                                 -> Vec<PairHit> {
        self.pairs_impl(scoring, reads, min_span, max_span, pen_unpaired, seed_len, stride, max_occ, pad, None)
    }

    /// Mate rescue (`bg_seed_extend_pairs_rescue_batch`): `seed_extend_batch_pairs`, and where a pair's seeded candidates hold no
    /// proper combination, the other mate is aligned inside the insert window of each of a mate's best `max_anchors` (1 ..= 4)
    /// candidates; a rescued alignment below `min_score` is discarded.  `PairHit::rescued` says which mate was placed that way.
    pub fn seed_extend_batch_pairs_rescue<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], max_anchors: u32, min_score: i32,
                                                        min_span: u32, max_span: u32, pen_unpaired: i32, seed_len: u32, stride: u32,
                                                        max_occ: u32, pad: u32)
                                                        -> Vec<PairHit> {
        let rp = sys::bg_rescue_params_t { max_anchors, min_score };
        self.pairs_impl(scoring, reads, min_span, max_span, pen_unpaired, seed_len, stride, max_occ, pad, Some(rp))
    }

    /// Read pairs with a mapping quality per mate (`bg_seed_extend_pairs_mapq_batch`): what `seed_extend_batch_pairs` returns, and
    /// for every pair a `PairQuality`.  A candidate below `min_score` is no alternative placement; `mapq_cap` is 0 ..= 254.
    pub fn seed_extend_batch_pairs_mapq<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], min_score: i32, mapq_cap: u32,
                                                      min_span: u32, max_span: u32, pen_unpaired: i32, seed_len: u32, stride: u32,
                                                      max_occ: u32, pad: u32)
                                                      -> Vec<(PairHit, PairQuality)> {
        assert!(reads.len() % 2 == 0, "mates come in pairs: an odd number of reads");
        assert!(mapq_cap <= 254, "mapq_cap outside 0 ..= 254");
        let table = tabulate(scoring);
        let sc = scoring_to_c(scoring, &table);
        let prm = sys::bg_seed_params_t { seed_len, stride, max_occ, pad };
        let pp = sys::bg_pair_params_t { min_span, max_span, pen_unpaired };
        let qp = sys::bg_pairq_params_t { min_score, mapq_cap };
        let (buf, off) = concat(reads);
        let n_pairs = reads.len() / 2;
        let zero = sys::bg_seed_hit_t { aln: zero_alignment(), window_start: 0, ref_start: 0, ref_end: 0, n_candidates: 0, n_seed_hits: 0 };
        let mut hits = vec![zero; reads.len()];
        let mut strand = vec![0u8; reads.len()];
        let mut pairs = vec![sys::bg_pair_hit_t { span: 0, n_proper: 0, proper: 0, reserved: [0; 3] }; n_pairs.max(1)];
        let mut multi = vec![sys::bg_multi_hit_t { sub_score: 0, n_loci: 0, n_reported: 0, mapq: 0, reserved: [0; 6] }; reads.len().max(1)];
        let mut ops = vec![0u8; 2 * buf.len() + (2 * pad as usize + 4) * reads.len() + 8];
        let mut used = 0u64;
        let rc = unsafe {
            sys::bg_seed_extend_pairs_mapq_batch(self.h, &sc, &prm, &pp, &qp, n_pairs as u64, buf.as_ptr(), off.as_ptr(), hits.as_mut_ptr(),
                                                 strand.as_mut_ptr(), pairs.as_mut_ptr(), multi.as_mut_ptr(), ops.as_mut_ptr(),
                                                 ops.len() as u64, &mut used)
        };
        assert!(rc == 0, "{}", strerror(rc));
        let hit = |r: usize| Hit {
            alignment: if hits[r].aln.score == sys::BG_MIN_SCORE { None } else { Some(to_alignment(&hits[r].aln, &ops)) },
            ref_start: hits[r].ref_start as usize,
            ref_end: hits[r].ref_end as usize,
            n_candidates: hits[r].n_candidates,
            reverse: strand[r] as i32 == sys::BG_HIT_REVERSE,
        };
        (0..n_pairs)
            .map(|p| {
                let (a, b) = (&multi[2 * p], &multi[2 * p + 1]);
                (PairHit { mates: [hit(2 * p), hit(2 * p + 1)], proper: pairs[p].proper != 0, span: pairs[p].span, n_proper: pairs[p].n_proper,
                           rescued: 0 },
                 PairQuality { mapq: [a.mapq, b.mapq], sub_score: [a.sub_score, b.sub_score], n_loci: [a.n_loci, b.n_loci] })
            })
            .collect()
    }

    /// Mate rescue with a mapping quality per mate (`bg_seed_extend_pairs_rescue_mapq_batch`): what `seed_extend_batch_pairs_rescue`
    /// returns, and for every pair a `PairQuality`; the mates of a rescued pair are judged against the pair's other accepted rescues
    /// and the mates' seeded candidates elsewhere.  `rescue_min_score` discards a rescued alignment, `min_score` an alternative.
    pub fn seed_extend_batch_pairs_rescue_mapq<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], max_anchors: u32,
                                                             rescue_min_score: i32, min_score: i32, mapq_cap: u32, min_span: u32,
                                                             max_span: u32, pen_unpaired: i32, seed_len: u32, stride: u32, max_occ: u32,
                                                             pad: u32)
                                                             -> Vec<(PairHit, PairQuality)> {
        assert!(reads.len() % 2 == 0, "mates come in pairs: an odd number of reads");
        assert!(mapq_cap <= 254, "mapq_cap outside 0 ..= 254");
        let table = tabulate(scoring);
        let sc = scoring_to_c(scoring, &table);
        let prm = sys::bg_seed_params_t { seed_len, stride, max_occ, pad };
        let pp = sys::bg_pair_params_t { min_span, max_span, pen_unpaired };
        let rp = sys::bg_rescue_params_t { max_anchors, min_score: rescue_min_score };
        let qp = sys::bg_pairq_params_t { min_score, mapq_cap };
        let (buf, off) = concat(reads);
        let n_pairs = reads.len() / 2;
        let zero = sys::bg_seed_hit_t { aln: zero_alignment(), window_start: 0, ref_start: 0, ref_end: 0, n_candidates: 0, n_seed_hits: 0 };
        let mut hits = vec![zero; reads.len()];
        let mut strand = vec![0u8; reads.len()];
        let mut pairs = vec![sys::bg_pair_hit_t { span: 0, n_proper: 0, proper: 0, reserved: [0; 3] }; n_pairs.max(1)];
        let mut rescued = vec![0u8; n_pairs.max(1)];
        let mut multi = vec![sys::bg_multi_hit_t { sub_score: 0, n_loci: 0, n_reported: 0, mapq: 0, reserved: [0; 6] }; reads.len().max(1)];
        // (a rescued hit has up to read + max_span operations)
        let mut ops = vec![0u8; 2 * buf.len() + (2 * pad as usize + 4 + max_span as usize) * reads.len() + 8];
        let mut used = 0u64;
        let rc = unsafe {
            sys::bg_seed_extend_pairs_rescue_mapq_batch(self.h, &sc, &prm, &pp, &rp, &qp, n_pairs as u64, buf.as_ptr(), off.as_ptr(),
                                                        hits.as_mut_ptr(), strand.as_mut_ptr(), pairs.as_mut_ptr(), rescued.as_mut_ptr(),
                                                        multi.as_mut_ptr(), ops.as_mut_ptr(), ops.len() as u64, &mut used)
        };
        assert!(rc == 0, "{}", strerror(rc));
        let hit = |r: usize| Hit {
            alignment: if hits[r].aln.score == sys::BG_MIN_SCORE { None } else { Some(to_alignment(&hits[r].aln, &ops)) },
            ref_start: hits[r].ref_start as usize,
            ref_end: hits[r].ref_end as usize,
            n_candidates: hits[r].n_candidates,
            reverse: strand[r] as i32 == sys::BG_HIT_REVERSE,
        };
        (0..n_pairs)
            .map(|p| {
                let (a, b) = (&multi[2 * p], &multi[2 * p + 1]);
                (PairHit { mates: [hit(2 * p), hit(2 * p + 1)], proper: pairs[p].proper != 0, span: pairs[p].span, n_proper: pairs[p].n_proper,
                           rescued: rescued[p] },
                 PairQuality { mapq: [a.mapq, b.mapq], sub_score: [a.sub_score, b.sub_score], n_loci: [a.n_loci, b.n_loci] })
            })
            .collect()
    }

    fn pairs_impl<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], min_span: u32, max_span: u32, pen_unpaired: i32,
                                seed_len: u32, stride: u32, max_occ: u32, pad: u32, rp: Option<sys::bg_rescue_params_t>)
                                -> Vec<PairHit> {
        assert!(reads.len() % 2 == 0, "mates come in pairs: an odd number of reads");
        let table = tabulate(scoring);
        let sc = scoring_to_c(scoring, &table);
        let prm = sys::bg_seed_params_t { seed_len, stride, max_occ, pad };
        let pp = sys::bg_pair_params_t { min_span, max_span, pen_unpaired };
        let (buf, off) = concat(reads);
        let n_pairs = reads.len() / 2;
        let zero = sys::bg_seed_hit_t { aln: zero_alignment(), window_start: 0, ref_start: 0, ref_end: 0, n_candidates: 0, n_seed_hits: 0 };
        let mut hits = vec![zero; reads.len()];
        let mut strand = vec![0u8; reads.len()];
        let mut pairs = vec![sys::bg_pair_hit_t { span: 0, n_proper: 0, proper: 0, reserved: [0; 3] }; n_pairs.max(1)];
        let mut rescued = vec![0u8; n_pairs.max(1)];
        // (a rescued hit has up to read + max_span operations)
        let window = 2 * pad as usize + 4 + if rp.is_some() { max_span as usize } else { 0 };
        let mut ops = vec![0u8; 2 * buf.len() + window * reads.len() + 8];
        let mut used = 0u64;
        let rc = unsafe {
            match &rp {
                Some(rp) => sys::bg_seed_extend_pairs_rescue_batch(self.h, &sc, &prm, &pp, rp, n_pairs as u64, buf.as_ptr(), off.as_ptr(),
                                                                   hits.as_mut_ptr(), strand.as_mut_ptr(), pairs.as_mut_ptr(),
                                                                   rescued.as_mut_ptr(), ops.as_mut_ptr(), ops.len() as u64, &mut used),
                None => sys::bg_seed_extend_pairs_batch(self.h, &sc, &prm, &pp, n_pairs as u64, buf.as_ptr(), off.as_ptr(), hits.as_mut_ptr(),
                                                        strand.as_mut_ptr(), pairs.as_mut_ptr(), ops.as_mut_ptr(), ops.len() as u64, &mut used),
            }
        };
        assert!(rc == 0, "{}", strerror(rc));
        let hit = |r: usize| Hit {
            alignment: if hits[r].aln.score == sys::BG_MIN_SCORE { None } else { Some(to_alignment(&hits[r].aln, &ops)) },
            ref_start: hits[r].ref_start as usize,
            ref_end: hits[r].ref_end as usize,
            n_candidates: hits[r].n_candidates,
            reverse: strand[r] as i32 == sys::BG_HIT_REVERSE,
        };
        (0..n_pairs)
            .map(|p| PairHit { mates: [hit(2 * p), hit(2 * p + 1)], proper: pairs[p].proper != 0, span: pairs[p].span, n_proper: pairs[p].n_proper,
                               rescued: if rp.is_some() { rescued[p] } else { 0 } })
            .collect()
    }

    /// Runner-up loci and MAPQ: up to `max_hits` (1 ..= 8) loci per read on both strands, the best first (`hits[0]` is what
    /// `seed_extend_batch_strands` reports).  A candidate below `min_score` is neither reported nor counted as a runner-up.
    pub fn seed_extend_batch_multi<F: MatchFunc>(&self, scoring: &Scoring<F>, reads: &[&[u8]], max_hits: u32, min_score: i32, mapq_cap: u32,
                                                 seed_len: u32, stride: u32, max_occ: u32, pad: u32)
                                                 -> Vec<MultiHit> {
        assert!(max_hits >= 1 && max_hits as i32 <= sys::BG_SEED_MAX_HITS, "max_hits outside 1 ..= 8");
        let table = tabulate(scoring);
        let sc = scoring_to_c(scoring, &table);
        let prm = sys::bg_seed_params_t { seed_len, stride, max_occ, pad };
        let mp = sys::bg_multi_params_t { max_hits, min_score, mapq_cap };
        let (buf, off) = concat(reads);
        let k = max_hits as usize;
        let zero = sys::bg_seed_hit_t { aln: zero_alignment(), window_start: 0, ref_start: 0, ref_end: 0, n_candidates: 0, n_seed_hits: 0 };
        let mut hits = vec![zero; reads.len() * k];
        let mut strand = vec![0u8; reads.len() * k];
        let mut multi = vec![sys::bg_multi_hit_t { sub_score: 0, n_loci: 0, n_reported: 0, mapq: 0, reserved: [0; 6] }; reads.len().max(1)];
        let mut ops = vec![0u8; k * (2 * buf.len() + (2 * pad as usize + 4) * reads.len() + 8)];
        let mut used = 0u64;
        let rc = unsafe {
            sys::bg_seed_extend_multi_batch(self.h, &sc, &prm, &mp, sys::BG_STRAND_BOTH as u32, reads.len() as u64, buf.as_ptr(), off.as_ptr(),
                                            hits.as_mut_ptr(), strand.as_mut_ptr(), multi.as_mut_ptr(), ops.as_mut_ptr(), ops.len() as u64,
                                            &mut used)
        };
        assert!(rc == 0, "{}", strerror(rc));
        let hit = |s: usize| Hit {
            alignment: Some(to_alignment(&hits[s].aln, &ops)),
            ref_start: hits[s].ref_start as usize,
            ref_end: hits[s].ref_end as usize,
            n_candidates: hits[s].n_candidates,
            reverse: strand[s] as i32 == sys::BG_HIT_REVERSE,
        };
        (0..reads.len())
            .map(|r| MultiHit {
                hits: (0..multi[r].n_reported as usize).map(|j| hit(r * k + j)).collect(),
                mapq: multi[r].mapq,
                sub_score: multi[r].sub_score,
                n_loci: multi[r].n_loci,
            })
            .collect()
    }
}
