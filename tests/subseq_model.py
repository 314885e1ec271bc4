"""The rule of `lexicmap utils subseq` / `utils genome-seqs` in plain Python, over the records of genome_build_fixture
(records() / concatenation()): what lm_index_subseqs, lm_index_subseq_rows, lm_index_genome_seqs and lm_format_subseqs are
held to (tests/test_subseq_plan_cpu.py without a GPU, tests/test_gpu_subseq.py on one).

  subseq2_literal / subseq_literal   the clamps of genome.go SubSeq2 (:1180-1191, 1297-1326, 1350) and SubSeq (:728-736),
                                     restated line by line
  contig_window / concat_window      the short form the library's planner uses (lm_subseq_plan.h)
  Model                              records, name resolution (subseq.go:371, 403-423, 582-605), extraction, genome_seqs
  fasta                              the text (subseq.go:204-205, 447-450, 632-636; util.go:311-347)
"""
import genome_build_fixture as F

OK, NO_GENOME, NO_SEQ, OUT_OF_RANGE, NOT_LOCAL = range(5)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def flanks(begin, end, rc, upstream, downstream):
    """subseq.go:388-397, 569-578"""
    if not rc:
        e_start = begin - upstream
        e_end = end + downstream
    else:
        e_start = begin - downstream
        e_end = end + upstream
    if e_start < 1:
        e_start = 1
    return e_start, e_end


def subseq2_literal(n_bases, contigs, interval, seqid, start, end):
    """genome.go:1180-1191, 1297-1326, 1350.  contigs: (id, size) of the record; start / end 0-based inclusive, as subseq.go
    passes them (eStart - 1, eEnd - 1).  -> (start in the record, bases, returned end) or None: seqid not found"""
    start0, end0 = start, end                   # :1180
    end_r = end                                 # :1181
    if start < 0:                               # :1183
        start = 0
    if end >= n_bases - 1:                      # :1186
        end = n_bases - 1
    if end < start:                             # :1189
        end = start
    found = False
    len_sum = seq_len = end_s = 0
    for cid, size in contigs:
        if cid == seqid:                        # :1297
            found = True
            seq_len = size
            start += len_sum
            end += len_sum
            end_s = len_sum + seq_len - 1       # :1303
        else:
            len_sum += size
            len_sum += interval
    if not found:                               # :1312
        return None
    if end0 >= seq_len:                         # :1320
        end = end_s
        end_r = seq_len - 1
    if start0 > seq_len:                        # :1324: the genome comes back with an empty sequence
        return start, 0, end_r
    length = end - start + 1                    # :1350
    return start, length, end_r


def subseq_literal(n_bases, start, end):
    """genome.go:728-736 (0-based inclusive) -> (start, bases)"""
    if start < 0:
        start = 0
    if end >= n_bases - 1:
        end = n_bases - 1
    if end < start:
        end = start
    return start, end - start + 1


def contig_window(sizes, ci, interval, e_start, e_end):
    """the short form: (0-based start in the record, bases, reported end)"""
    off = sum(sizes[:ci]) + ci * interval
    seq_len = sizes[ci]
    end = min(e_end, seq_len)
    return off + e_start - 1, (0 if e_start > seq_len else end - e_start + 1), end


def concat_window(rec_len, e_start, e_end):
    """(status, 0-based start, bases, reported end): beyond the record is OUT_OF_RANGE, the clamped end is reported"""
    end = min(e_end, rec_len)
    if e_start > rec_len:
        return OUT_OF_RANGE, 0, 0, end
    return OK, e_start - 1, end - e_start + 1, end


def find_seq(ids, seq_id):
    """contig number, -1: none, -2: the id occurs twice in the record"""
    hits = [i for i, x in enumerate(ids) if x == seq_id]
    return -1 if not hits else hits[0] if len(hits) == 1 else -2


def resolve(recs_ids, seq_id, seq_idx):
    """recs_ids: the contig ids of the genome's records in chunk order -> (record in the list, contig, status)"""
    if not recs_ids:
        return -1, -1, NO_GENOME
    if not seq_id:
        if seq_idx >= 0:
            return (0, -1, NO_SEQ) if seq_idx >= len(recs_ids[0]) else (0, seq_idx, OK)
        return 0, -1, OK
    for r, ids in enumerate(recs_ids):
        f = find_seq(ids, seq_id)
        if f == -1:
            continue
        return (r, f, OK) if f >= 0 else (r, -1, NO_SEQ)
    return -1, -1, NO_SEQ


def wrap(s, width):
    """util.go:311-347"""
    if width < 1 or not s:
        return bytes(s)
    return b"\n".join(s[i:i + width] for i in range(0, len(s), width))


ROW_KEYS = ("query", None, None, "sgenome", "sseqid", "qcovGnm", "cls", "hsp", "qcovHSP", "alenHSP", "pident", "gaps", "qstart",
            "qend", "sstart", "send", "sstr", "slen", "evalue", "bitscore")


def header(name, begin, end, rc, tsv=None):
    """subseq.go:632-636; with the row's TSV line (20 columns) the long header of :204-205, 447-450"""
    h = ">%s:%d-%d:%s" % (name, begin, end, "-" if rc else "+")
    if tsv is not None:
        cols = tsv.split("\t")
        h += "".join(" %s=%s" % (k, c) for k, c in zip(ROW_KEYS, cols) if k)
    return h


class Model:
    """records: [(genome id, [(contig id, bases)])] in record order; keys[i]: the key of record i (default: batch 0)"""

    def __init__(self, gs=None, keys=None, interval=F.CONTIG_INTERVAL, records=None):
        self.records = records if records is not None else F.records(gs if gs is not None else F.genomes())
        self.interval = interval
        self.keys = list(keys) if keys is not None else list(range(len(self.records)))
        self.concat = [F.concatenation(c, interval) for _, c in self.records]
        self.ids = [[cid for cid, _ in c] for _, c in self.records]
        self.sizes = [[len(s) for _, s in c] for _, c in self.records]
        self.of_key = {k: i for i, k in enumerate(self.keys)}

    def records_of(self, genome_id):
        return [i for i, (g, _) in enumerate(self.records) if g == genome_id]

    def one(self, region, upstream=0, downstream=0, local=None):
        """region: dict as Index.subseq takes it -> dict(status, key, seq_idx, rc, begin, end, seq, genome_id, seq_id);
        local: the record numbers this shard holds (None: all)"""
        rc = bool(region.get("rc"))
        e_start, e_end = flanks(region["begin"], region["end"], rc, upstream, downstream)
        out = dict(status=OK, key=0, seq_idx=-1, rc=int(rc), begin=e_start, end=e_end, seq=b"", genome_id=None, seq_id=None)
        seq_id, seq_idx = region.get("seq_id"), region.get("seq_idx", -1)
        if region.get("key") is None:
            recs = [r for r in self.records_of(region.get("genome_id")) if local is None or r in local]
            r, ci, st = resolve([self.ids[x] for x in recs], seq_id, seq_idx)
            rec = recs[r] if r >= 0 else -1
        else:
            out["key"] = region["key"]
            rec = self.of_key.get(region["key"], -1)
            if rec < 0:
                return dict(out, status=NO_GENOME)
            if local is not None and rec not in local:
                return dict(out, status=NOT_LOCAL)
            ci, st = -1, OK
            if seq_id:
                ci = find_seq(self.ids[rec], seq_id)
                if ci < 0:
                    ci, st = -1, NO_SEQ
            elif seq_idx >= 0:
                ci, st = (seq_idx, OK) if seq_idx < len(self.ids[rec]) else (-1, NO_SEQ)
        if rec >= 0:
            out.update(key=self.keys[rec], genome_id=self.records[rec][0])
        if st != OK:
            return dict(out, status=st)
        if ci >= 0:
            src, n, end = contig_window(self.sizes[rec], ci, self.interval, e_start, e_end)
            out.update(seq_idx=ci, seq_id=self.ids[rec][ci])
        else:
            st, src, n, end = concat_window(len(self.concat[rec]), e_start, e_end)
            if st != OK:
                return dict(out, status=st, end=end)
        s = self.concat[rec][src:src + n]
        assert len(s) == n
        return dict(out, end=end, seq=revcomp(s) if rc else s)

    def run(self, regions, upstream=0, downstream=0, local=None):
        return [self.one(r, upstream, downstream, local) for r in regions]

    def genome_seqs(self, genome_id):
        """genome-seqs.go:115-137: (contig id, bases as stored) in record and contig order"""
        out = []
        for r in self.records_of(genome_id):
            at = 0
            for cid, size in zip(self.ids[r], self.sizes[r]):
                out.append((cid, self.concat[r][at:at + size]))
                at += size + self.interval
        return out

    def row_region(self, row):
        """the region of a search row (dict or numpy record): lm_index_subseq_rows"""
        return dict(key=int(row["batch_genome"]), seq_idx=int(row["seq_idx"]), begin=int(row["tbegin"]) + 1, end=int(row["tend"]) + 1,
                    rc=int(row["rc"]))


def fasta(answers, width, tsv=None, genome_seqs=False):
    """the text of lm_format_subseqs for Model.run's answers; tsv: the rows' TSV lines (the long header)"""
    out = []
    for i, a in enumerate(answers):
        if a["status"] != OK:
            continue
        if genome_seqs:
            h = ">" + a["seq_id"]
        else:
            h = header(a["seq_id"] if a["seq_idx"] >= 0 else a["genome_id"], a["begin"], a["end"], a["rc"], tsv[i] if tsv else None)
        out.append(h.encode() + b"\n" + wrap(a["seq"], width) + b"\n")
    return b"".join(out)
