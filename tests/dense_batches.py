"""Batches dense in short reads and in ORFs, and the preconditions that prove they reach the per-tile, per-wave and per-round caps
of the kernels (tests/test_dense_batches_host.py asserts them without a GPU, tests/test_gpu_dense_batches.py before every device
call).  Every batch comes from a seeded numpy generator; every precondition is computed from the read offsets or from the CPU
oracle alone, never from device output, and raises AssertionError when it does not hold.

  cap                                          batch that passes it         precondition
  MG_TILE_READS 64 reads per tile              short_ragged(_long)          require_front_half_tiles: mg_plan's windows restated
  MT_NC 6 reads per tile with per-read nulls   the same, short_uniform      require_front_half_tiles (nulls=True); 504 // L > 6
  MT_ORFS 64 ORFs per pass of a tile           short_ragged(_long)          require_front_half_tiles: the oracle's ORFs per tile
  ET_MAXR 64 reads, ET_MAXO 192 ORFs per tile  short_ragged, -i / -s        require_error_tiles: k_et_tiles restated
  EW_MAXO 64 ORFs of one (read, strand)        orf_dense                    require_orf_dense
  OB_GROUP 10 reads of a window                short_ragged(_long)          require_orfbits_window
  NR_MAX 384 reads of a round of string sums   NOT REACHED, by no batch     require_strings_full_rounds: a round is 14 chunks of
                                                                            2,048 bases, 335 reads of 86 bases at the most;
                                                                            strings_86_rounds fills such rounds (334 or 335 reads)
  SEL_R 32 reads of a 1,024-base tile          selection()                  require_selection
  eight reads per block of k_frame6p, all heads  short_uniform(1 .. 3)      require_all_heads
"""
import numpy as np

BASES = np.frombuffer(b"acgt", np.uint8)
MG_KW = dict(min_gene_len=6, ignore_score_len=12)                 # the front half on reads this short (allow_truncated is the default)
UNIFORM_LENGTHS = (1, 2, 3, 11, 12, 13, 40)
REPEAT_A = "atgctaacgcttccgtag"                                   # x 53: 106 forward and 55 reverse ORFs kept (Min_Gene_Len 6, Min_Indel_ORF_Len 15)
REPEAT_B = "atggtatcggctacctag"                                   # x 53: 55 forward and 105 reverse
REPEAT_COUNTS = {REPEAT_A: (106, 55, 58, 112), REPEAT_B: (55, 105, 57, 110)}   # (forward, reverse, starts of the whole read's -i lists, of its -s lists)


def random_reads(rng, lengths, at=0.25):
    """reads of the given lengths; at: the frequency of a and of t each (0.25: uniform)"""
    if at == 0.25:
        return [BASES[rng.integers(0, 4, size=int(n))].tobytes().decode() for n in lengths]
    p = [at, 0.5 - at, 0.5 - at, at]
    return [BASES[rng.choice(4, size=int(n), p=p)].tobytes().decode() for n in lengths]


def revcomp(s):
    return s[::-1].translate(str.maketrans("acgt", "tgca"))


def offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


# ---------------------------------------------------------------- the batches

def short_ragged():
    """1,500 reads of 0 .. 8 bases, then 1,500 of 9 .. 40; empty reads at both ends of the batch and in runs in both halves"""
    rng = np.random.default_rng(20240)
    a = rng.integers(0, 9, size=1500)
    b = rng.integers(9, 41, size=1500)
    a[:3] = 0
    a[700:723] = 0
    a[1499] = 0                                                    # (an empty read right before the first longer one)
    b[800:805] = 0
    b[-2:] = 0
    return random_reads(rng, np.concatenate([a, b]))


def short_ragged_long():
    """short_ragged with 40 reads of 300 .. 700 bases scattered through it: max_len, n_over_512 and the mean length change"""
    seqs = short_ragged()
    rng = np.random.default_rng(20241)
    at = np.sort(rng.choice(np.arange(1, len(seqs)), size=40, replace=False))     # (the empty reads stay first and last)
    longs = random_reads(rng, rng.integers(300, 701, size=40))
    for k in range(39, -1, -1):                                    # from the back: the earlier places stay where they are
        seqs.insert(int(at[k]), longs[k])
    return seqs


def short_uniform(L):
    assert L in UNIFORM_LENGTHS
    return random_reads(np.random.default_rng(20250 + L), [L] * 2000)


def orf_dense():
    """30 ordinary reads of 100 .. 900 bases mixed with eight reads that carry more than 64 kept ORFs on one strand: the two repeat
    reads, their reverse complements and four 960-base reads rich in a and t (0.45 each)"""
    rng = np.random.default_rng(20260)
    seqs = random_reads(rng, rng.integers(100, 901, size=30))
    dense = [REPEAT_A * 53, REPEAT_B * 53, revcomp(REPEAT_A * 53), revcomp(REPEAT_B * 53)] + random_reads(rng, [960] * 4, at=0.45)
    at = np.sort(rng.choice(len(seqs) + 1, size=len(dense), replace=False))
    for k in range(len(dense) - 1, -1, -1):
        seqs.insert(int(at[k]), dense[k])
    return seqs


def quality_12_percent(seqs, seed):
    """a quality file's values: 12 % of the bases below 19 (as tests/test_gpu_mg_err.py draws them) -> one int32 array per read"""
    rng = np.random.default_rng(seed)
    return [np.where(rng.random(len(s)) < 0.12, rng.integers(0, 19, len(s)), rng.integers(19, 41, len(s))).astype(np.int32) for s in seqs]


def strings_86():
    """900 reads of 86 bases with one of 87 or 88 at every 50th place: not uniform, min_len 86, about 78,000 bases"""
    rng = np.random.default_rng(20270)
    lens = np.full(900, 86)
    lens[49::50] = 87 + (np.arange(len(lens[49::50])) & 1)
    return random_reads(rng, lens)


def strings_85():
    """strings_86 with one read cut to 85 bases: the two-pass form"""
    seqs = strings_86()
    seqs[431] = seqs[431][:85]
    return seqs


def strings_86_rounds():
    """92,000 reads of 86 bases with one of 87 or 88 at every 50th place, 7.9 M bases: 3,864 chunks of 2,048 bases, so that each of
    up to 256 work-groups of the fused string sums gets 16 consecutive chunks or more -- a full round of 14 and a partial one"""
    rng = np.random.default_rng(20271)
    lens = np.full(92000, 86)
    lens[49::50] = 87 + (np.arange(len(lens[49::50])) & 1)
    off = np.concatenate([[0], np.cumsum(lens)])
    text = BASES[rng.integers(0, 4, size=int(off[-1]))].tobytes().decode()
    return [text[a:b] for a, b in zip(off[:-1], off[1:])]


def selection(n_source):
    """5,000 indices into a batch of n_source reads: repeats, runs of one read, runs of the batch's empty reads (the caller's
    precondition finds them), neighbours in reverse order"""
    rng = np.random.default_rng(20280)
    idx = rng.integers(0, n_source, size=5000)
    idx[100:140] = 0                                               # read 0 is empty in short_ragged
    idx[141:150] = idx[140]                                        # the same read nine times
    idx[2000:2064] = np.arange(763, 699, -1)                       # the run of empty reads 700 .. 722 and its neighbours, backwards
    idx[-3:] = [n_source - 1, 0, n_source - 3]                      # an empty read last but one
    return idx.astype(np.uint64)


def training_strings():
    """3,000 training strings of 0 .. 15 bases (bytes, as gmg_icm_train and the oracle take them)"""
    rng = np.random.default_rng(20290)
    return [s.encode() for s in random_reads(rng, rng.integers(0, 16, size=3000))]


# ---------------------------------------------------------------- counting, from offsets alone

def most_starts_in_a_stretch(seqs, width, nonempty=True):
    """the largest number of reads (nonempty: of non-empty reads) that begin inside one stretch of `width` bases, over the
    stretches that begin where a read begins"""
    off = offsets(seqs)
    begin = off[:-1][np.diff(off) > 0] if nonempty else off[:-1]
    if len(begin) == 0:
        return 0
    return int((np.searchsorted(begin, begin + width, side="left") - np.arange(len(begin))).max())


def fewest_starts_in_a_stretch(seqs, width, lo, hi):
    """the smallest number of non-empty reads that begin inside one stretch of `width` bases, over EVERY stretch that lies inside
    the bases lo .. hi of the batch: whatever the tile windows' phase, each of them in that range holds that many"""
    off = offsets(seqs)
    begin = off[:-1][np.diff(off) > 0]
    at = np.arange(lo, hi - width + 1)
    return int((np.searchsorted(begin, at + width, side="left") - np.searchsorted(begin, at, side="left")).min())


def most_reads_in_an_aligned_piece(seqs, size, overlap=False):
    """the largest number of non-empty reads that begin in (overlap: that have a base in) one piece [k size, (k + 1) size) of the batch"""
    off = offsets(seqs)
    keep = np.diff(off) > 0
    b, e = off[:-1][keep], off[1:][keep]
    if len(b) == 0:
        return 0
    n_pieces = int(off[-1] + size - 1) // size
    first = b // size
    last = (e - 1) // size if overlap else first
    cnt = np.zeros(n_pieces + 1, np.int64)
    np.add.at(cnt, first, 1)
    np.add.at(cnt, last + 1, -1)
    return int(np.cumsum(cnt)[:n_pieces].max())


def orfs_per_read(oracle, seqs, err, **kw):
    """Find_Orfs' records per read by the oracle; err: with the Min_Indel_ORF_Len 15 rule of the error branch"""
    prm = oracle.mg_params(**kw)
    find = (lambda s: oracle.find_orfs_err(s, prm, 15)) if err else (lambda s: oracle.find_orfs(s, prm))
    return [find(s) for s in seqs]


def strand_counts(orfs):
    """(forward, reverse) records of one read"""
    return int((orfs[:, 0] > 0).sum()), int((orfs[:, 0] < 0).sum())


# ---------------------------------------------------------------- how the library cuts a batch, restated from the offsets

def front_half_plan(seqs, nulls=False, fused=True, forced_tile=0, gene32=True):
    """mg_plan's tiling of a ragged batch in the default mode -> (tile_window, cap, reads per tile at the most).  nulls: a null model
    per read; fused / forced_tile / gene32: the options mg_fused, mg_tile (0, 1, 2, 4) and whether the call's table has the GENE32 form"""
    lens = np.array([len(s) for s in seqs], np.int64)
    n, total, max_len, over = len(lens), int(lens.sum()), int(lens.max()), int((lens > 512).sum())
    assert len(set(lens.tolist())) > 1 and total > 0
    nw = 0
    if fused:
        if forced_tile in (1, 2, 4):
            nw = forced_tile
        else:
            nw = 1 if (max_len <= 567 or over * 10 <= n) else 2 if max_len <= 2 * 567 else 4
            if (total // n) * (6 if nulls else 64) * 5 >= 4 * 567 * 4:
                nw = 4
        cap = 63 * (8 if max_len <= 504 * nw else 9) * nw
    else:
        small = forced_tile == 512 if forced_tile else (max_len <= 512 or over * 10 <= n)
        cap = 512 if small else 1504
    reads_max = 6 if (nw and nulls and gene32) else 64
    return cap - min(max_len, cap // 2), cap, reads_max


def front_half_tiles(seqs, window, cap, reads_max):
    """mg_tile_reads for every window: (first read, reads that begin in the window, reads the tile takes); empty reads count"""
    off = offsets(seqs)
    n, total = len(off) - 1, int(off[-1])
    out = []
    for k in range(total // window + 1):
        first = min(int(np.searchsorted(off, k * window, side="left")), n)
        end = min(int(np.searchsorted(off, (k + 1) * window, side="left")), n)
        nfit = 0
        while first + nfit < end and nfit < reads_max and off[first + nfit + 1] - off[first] <= cap:
            nfit += 1
        out.append((first, end - first, nfit))
    return out


def error_tiles(seqs, cap=1536, reads_max=64, chunk_tiles=16):
    """k_et_tiles: greedy runs of consecutive reads, closed by the ET_MAXR-th read, by a read that would pass `cap` bases or by the end
    of a chunk of chunk_tiles * cap bases; reads beyond cap bases stay out -> [(first read, reads)]"""
    off = offsets(seqs)
    n, total, chunk = len(off) - 1, int(off[-1]), cap * chunk_tiles
    n_chunks = total // chunk + 1
    out = []
    for k in range(n_chunks):
        r0 = min(int(np.searchsorted(off, k * chunk, side="left")), n)
        r1 = n if k + 1 == n_chunks else min(int(np.searchsorted(off, (k + 1) * chunk, side="left")), n)
        first = nfit = 0
        for r in range(r0, r1):
            if off[r + 1] - off[r] > cap:
                if nfit:
                    out.append((first, nfit))
                nfit = 0
                continue
            if nfit and (nfit == reads_max or off[r + 1] - off[first] > cap):
                out.append((first, nfit))
                nfit = 0
            if not nfit:
                first = r
            nfit += 1
        if nfit:
            out.append((first, nfit))
    return out


def string_sum_rounds(seqs, n_cu=256):
    """the rounds of the fused string sums (k_frame6t in its SUM form, launched by gmg_launch_strings_sum): min(n_cu, n_chunks)
    work-groups, each with ceil(n_chunks / work-groups) consecutive chunks of 2,048 bases, 14 chunks per round
    -> [(chunks of the round, reads that have a base in it)].  n_cu: the device's compute units, 256 on an MI355X; fewer only
    make a work-group's share longer"""
    off = offsets(seqs)
    n_chunks = int(off[-1]) // 2048
    if n_chunks == 0:
        return []
    grid = min(n_cu, n_chunks)
    per_worker = (n_chunks + grid - 1) // grid
    out = []
    for w in range(grid):
        chunk0 = w * per_worker
        if chunk0 >= n_chunks:
            break
        n_mine = min(per_worker, n_chunks - chunk0)
        for j0 in range(0, n_mine, 14):
            kk = min(14, n_mine - j0)
            g0, g1 = (chunk0 + j0) * 2048, (chunk0 + j0 + kk) * 2048
            first = int(np.searchsorted(off, g0, side="right")) - 1
            last = int(np.searchsorted(off, g1, side="left")) - 1
            out.append((kk, last - first + 1))
    return out


# ---------------------------------------------------------------- the preconditions

def require_short_ragged(seqs):
    """the density of the batch: more than 64 reads begin inside some 400-base stretch (in every one of the first 5,000 bases when
    no read is long); more than 150 reads in some 2,048-base chunk of the six-frame pass and of the ORF records' scan; more than
    32 in some 1,024-base tile (the tile table of the batch); empty reads first, last and in runs.  What the tiles of the front half
    and of the error branch hold is require_front_half_tiles' and require_error_tiles' business"""
    lens = np.array([len(s) for s in seqs])
    assert lens[0] == 0 and lens[-1] == 0 and lens.min() == 0 and ((lens[1:] == 0) & (lens[:-1] == 0)).sum() >= 20
    most = most_starts_in_a_stretch(seqs, 400)
    assert most > 64, most
    if lens.max() <= 40:
        every = fewest_starts_in_a_stretch(seqs, 400, 0, 5000)
        assert every > 64, every
    chunk = most_reads_in_an_aligned_piece(seqs, 2048)
    assert chunk > 150, chunk
    tile = most_reads_in_an_aligned_piece(seqs, 1024)
    assert tile > 32, tile
    return dict(stretch400=most, chunk2048=chunk, tile1024=tile)


def require_short_ragged_long(seqs):
    """what short_ragged has, and the statistics that steer mg_plan elsewhere: a longest read beyond 567 bases (a one-wave tile),
    reads beyond 512 bases but fewer than a tenth, a mean length between the short batch's and a tile's"""
    got = require_short_ragged(seqs)
    lens = np.array([len(s) for s in seqs])
    assert 567 < lens.max() <= 700 and 0 < (lens > 512).sum() * 10 <= len(lens) and lens.min() == 0
    short = np.array([len(s) for s in short_ragged()])
    assert lens.mean() > 1.3 * short.mean()
    got.update(max_len=int(lens.max()), n_over_512=int((lens > 512).sum()), mean=float(lens.mean()))
    return got


def require_orfs_per_64_reads(oracle, seqs, err, **kw):
    """some 64 consecutive reads carry more than 192 ORF records (ET_MAXO of the error branch's tiles; three passes of MT_ORFS = 64
    in stages 3 and 4 of the fused tile kernel) -- by the oracle's Find_Orfs"""
    n = np.array([len(o) for o in orfs_per_read(oracle, seqs, err, **kw)], np.int64)
    c = np.concatenate([[0], np.cumsum(n)])
    most = int((c[64:] - c[:-64]).max())
    assert most > 192, most
    return dict(n_orfs=int(n.sum()), per_read=float(n.mean()), most_in_64_reads=most)


def require_front_half_tiles(oracle, seqs, nulls=False, **kw):
    """for every tiling the options mg_fused 0 / 1 x mg_tile 0 / 1 / 2 / 4 give this batch (front_half_plan), by mg_tile_reads restated:
    some window receives more reads than a tile may take and the tile closes at that number (the surplus goes to the per-lane
    kernel); with the default plan, some tile's reads carry more than MT_ORFS = 64 ORF records by the oracle (stages 3 and 4 loop)"""
    n_orfs = np.array([len(o) for o in orfs_per_read(oracle, seqs, False, **kw)], np.int64)
    c = np.concatenate([[0], np.cumsum(n_orfs)])
    got = {}
    for fused in (True, False):
        for forced in (0, 1, 2, 4):
            for g32 in ((True, False) if nulls and fused else (True,)):
                window, cap, reads_max = front_half_plan(seqs, nulls, fused, forced, g32)
                tiles = front_half_tiles(seqs, window, cap, reads_max)
                full = [t for t in tiles if t[1] > reads_max and t[2] == reads_max]
                assert len(full) > 0, (fused, forced, g32, window, cap, reads_max)
                most_orfs = max(int(c[f + k] - c[f]) for f, _, k in tiles)
                if fused and not forced and g32:
                    assert most_orfs > 64 or nulls, (window, most_orfs)
                    got = dict(window=window, cap=cap, reads_max=reads_max, full_tiles=len(full), tiles=len(tiles), most_orfs=most_orfs,
                               most_reads_in_a_window=max(t[1] for t in tiles))
    return got


def require_error_tiles(oracle, seqs, **kw):
    """the tiles of k_mg_err_tile (error_tiles): some are closed by their ET_MAXR = 64th read, and some hold more than ET_MAXO = 192 ORF
    records (Find_Orfs with the Min_Indel_ORF_Len rule, by the oracle), so that the records loop"""
    n_orfs = np.array([len(o) for o in orfs_per_read(oracle, seqs, True, **kw)], np.int64)
    c = np.concatenate([[0], np.cumsum(n_orfs)])
    tiles = error_tiles(seqs)
    assert sum(k for _, k in tiles) == len(seqs)
    by_reads = sum(1 for f, k in tiles if k == 64 and f + k < len(seqs))
    most = max(int(c[f + k] - c[f]) for f, k in tiles)
    assert by_reads > 0 and most > 192, (by_reads, most)
    return dict(tiles=len(tiles), closed_by_64_reads=by_reads, most_orfs=most)


def require_orfbits_window(seqs):
    """the bit-mask ORF finder's window of a ragged batch is 9.5 mean read lengths (mg_plan: total * 19 / 2 / n_reads bases) and a wave
    walks OB_GROUP = 10 reads at a time: some window holds the begins of more than 10 reads, empty ones included"""
    off = offsets(seqs)
    want = max(int(off[-1]) * 19 // 2 // (len(off) - 1), 1)
    most = int(np.bincount(off[:-1] // want).max())
    assert most > 10, (want, most)
    return dict(window=want, most=most)


def require_all_heads(seqs, model_len):
    """every base of every read is a partial-window head: no read reaches model_len - 1 bases, and there are more reads than the
    eight a block of the heads pass takes"""
    assert len(seqs) > 8 and 0 < max(len(s) for s in seqs) < model_len - 1


def require_orf_dense(oracle, seqs, **kw):
    """nloc of k_mg_err_wave / k_mg_err_wcount counts the ORF records of one (read, strand): at least four reads have more than
    EW_MAXO = 64 on a strand (the wave gives up and the batch repeats on the level kernels), at least one read has at most 64 on
    both -- and every read is short enough for a wave (960 bases), so that it is this overflow that moves the batch"""
    counts = [strand_counts(o) for o in orfs_per_read(oracle, seqs, True, **kw)]
    over = sum(1 for f, r in counts if max(f, r) > 64)
    under = sum(1 for f, r in counts if max(f, r) <= 64 and f + r > 0)
    assert over >= 4 and under >= 1, (over, under)
    assert max(len(s) for s in seqs) <= 960
    return dict(over=over, under=under, most=max(max(c) for c in counts))


def require_repeat_unit(oracle, unit, o_gene, o_indep):
    """the counts the two repeat units were chosen for, by the oracle with MG_KW: kept ORFs per strand (Min_Indel_ORF_Len 15; the
    last one of the weaker strand by Min_Gene_Len 6), starts of the whole read's -i lists (no homopolymer run of three:
    Set_Quality_454 marks nothing, the lists stay short) and of its -s lists; the reverse complement swaps the strands"""
    seq = unit * 53
    assert len(seq) == 954 and not any(c * 3 in seq for c in "acgt")
    prm = oracle.mg_params(**MG_KW)
    got = []
    for ekw in (dict(allow_indels=True), dict(allow_subs=True)):
        orfs, _, scored = oracle.mg_read_errors(o_gene, o_indep, seq.encode(), prm, oracle.mg_err_params(**ekw))
        got.append(strand_counts(orfs) + (sum(len(st) for _, st in scored),))
    fwd, rev = got[0][:2]
    assert got[1][:2] == (fwd, rev) and (fwd, rev, got[0][2], got[1][2]) == REPEAT_COUNTS[unit], got
    assert strand_counts(oracle.find_orfs_err(revcomp(seq), prm, 15)) == (rev, fwd)
    return fwd, rev, got[0][2], got[1][2]


def require_strings_round(seqs, fused):
    """fused: not uniform, no read below 86 bases, more than two rounds of 32,768 bases (the batch the issue asks for).  It opens the
    fused form on a ragged batch, whose rounds find their reads through s_roff -- but with 38 chunks and a work-group per chunk every
    round is ONE chunk of about 25 reads: this batch is nowhere near NR_MAX (see require_strings_full_rounds).  Not fused: one read
    of 85 bases.  -> the most reads a round overlaps"""
    lens = np.array([len(s) for s in seqs])
    assert len(set(lens)) > 1 and lens.sum() > 2 * 32768
    if fused:
        assert lens.min() == 86
    else:
        assert lens.min() == 85 and (lens == 85).sum() == 1
    return max(r for _, r in string_sum_rounds(seqs))


def require_strings_full_rounds(seqs):
    """a batch whose work-groups run FULL rounds of the fused string sums: 14 chunks, 28,672 bases.  With no read below 86 bases such
    a round overlaps 28,672 // 86 + 2 = 335 reads at the most, so NR_MAX = 384 cannot be reached and the branch beyond it (global
    atomics) stays untested; what is reached is the fullest s_roff / s_sum a call can have: 334 reads or more in some round.  Also
    partial rounds, and a last work-group with a shorter share"""
    lens = np.array([len(s) for s in seqs])
    assert len(set(lens)) > 1 and lens.min() == 86
    bound = 14 * 2048 // 86 + 2
    assert bound == 335 < 384
    for n_cu in (256, 128, 64):                                           # (MI355X: 256 compute units; fewer make the shares longer)
        rounds = string_sum_rounds(seqs, n_cu)
        most = max(r for _, r in rounds)
        assert 334 <= most <= bound, (n_cu, most)
        assert sum(1 for k, _ in rounds if k == 14) >= 100 and any(k < 14 for k, _ in rounds), n_cu
    return max(r for _, r in string_sum_rounds(seqs))


def require_selection(seqs, idx):
    """the selection has repeats, runs of empty reads, more than SEL_R = 32 reads in some 1,024-base tile of the NEW batch (in most of
    them) and a last tile that is partial, with a last word that is partial too"""
    idx = np.asarray(idx, np.int64)
    sel = [seqs[i] for i in idx]
    lens = np.array([len(s) for s in sel])
    total = int(lens.sum())
    assert len(idx) == 5000 and len(set(idx.tolist())) < len(idx)
    empty = lens == 0
    assert (empty[1:] & empty[:-1]).sum() >= 30 and empty[-2]
    assert total % 1024 != 0 and total % 16 != 0
    off = offsets(sel)
    per_tile = np.bincount(off[:-1][~empty] // 1024, minlength=(total + 1023) // 1024)
    assert per_tile.max() > 32 and (per_tile > 32).sum() * 2 > len(per_tile), per_tile
    return dict(total=total, most_per_tile=int(per_tile.max()))


def require_groups(seqs):
    """one group per read: some 2,048-base chunk holds reads of more than 50 groups"""
    most = most_reads_in_an_aligned_piece(seqs, 2048, overlap=True)
    assert most > 50, most
    return most


def require_training_strings(strings, model_len):
    """most strings are shorter than the window, some are empty, some reach it"""
    lens = np.array([len(s) for s in strings])
    assert len(lens) == 3000 and lens.max() == 15 and (lens == 0).sum() > 50 and (lens < model_len).sum() > 2000 and (lens >= model_len).sum() > 200
