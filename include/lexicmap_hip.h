/*
 * lexicmap_hip.h — C-ABI of the MI355X-native `lexicmap search` hot path (liblexicmap_hip.so).
 *
 * The reference (shenwei356/LexicMap) is pure Go built with CGO_ENABLED=0 and has no FFI of its own
 * (lexicmap/build.sh:7); this header is the seam a cgo shim in lexicmap/cmd would bind (INTEGRATION.md shows it).
 * Each entry point names the reference interface it replaces (paths relative to lexicmap/cmd/).
 *
 * Conventions
 *   - plain C types only; every function returns lm_status (0 = LM_OK) unless noted; lm_last_error() gives the text.
 *   - inputs are borrowed for the duration of the call (Go may move memory afterwards); outputs are callee-allocated
 *     and released with the matching *_free (mirrors the reference's Recycle* hand-back, lib-index-search.go:1170).
 *   - "no hit" is success with zero rows (the reference returns (nil,nil): lib-index-search.go:1669-1672).
 *   - the library needs a gfx950 GPU: every entry point that computes fails with LM_ERR_NO_DEVICE otherwise. There
 *     is no CPU fallback.
 */
#ifndef LEXICMAP_HIP_H
#define LEXICMAP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int lm_status;
enum {
    LM_OK = 0,
    LM_ERR_IO = 1,        /* missing / broken index file (reference: checkError -> exit, util-cli.go:35) */
    LM_ERR_FORMAT = 2,    /* magic / version mismatch (kv-data.go:54-64, genome.go:58-71) */
    LM_ERR_OPTION = 3,    /* option out of range (search.go:159-229, lib-index-search.go:483-485) */
    LM_ERR_NO_DEVICE = 4, /* no HIP device / not gfx950 */
    LM_ERR_HIP = 5,       /* HIP runtime error */
    LM_ERR_NOMEM = 6,
    LM_ERR_ARG = 7
};

/* Search options: IndexSearchingOptions (lib-index-search.go:57-106) + SeqComparatorOptions as wired by
 * search.go:305-382.  Defaults = the flag defaults of search.go:631-731. */
typedef struct lm_options {
    int32_t min_prefix;          /* -p/--seed-min-prefix 15 */
    int32_t min_single_prefix;   /* -P/--seed-min-single-prefix 17 */
    int32_t top_n_genomes;       /* -n 0 */
    int32_t top_n_chains;        /* -N 0 */
    double max_gap;              /* --seed-max-gap 50 */
    double max_distance;         /* --seed-max-dist 1000 */
    int32_t ext_len;             /* --align-ext-len 1000 */
    int32_t ext_len2;            /* 50, hard-coded at search.go:325 */
    double min_qcov_per_genome;  /* -Q 0 */
    double max_evalue;           /* -e 10 */
    int32_t output_seq;          /* -a/--all */
    int32_t align_max_gap;       /* --align-max-gap 20 */
    int32_t align_band;          /* --align-band 100 */
    int32_t align_min_match_len; /* -l 50 */
    double align_min_pident;     /* -i 70 */
    double min_qcov_per_hsp;     /* -q 0 */
    /* sharding of the genome set across ranks: this process loads genomes with
     * (dense genome number % shard_count) == shard_rank. shard_count <= 1 loads everything. */
    int32_t shard_rank, shard_count;
    int64_t total_bases_override; /* >0: e-value database size shared by all shards (info.toml input-bases) */
} lm_options;

typedef struct lm_index lm_index;

typedef struct lm_index_info {
    int32_t k, masks, mask_prefix, anchor_prefix;
    int64_t total_bases;   /* info.toml input-bases: the e-value database size (lib-index-search.go:1918) */
    int64_t genomes;       /* genomes resident on this device */
    int64_t seeds;         /* (k-mer,value) pairs resident on this device */
    int64_t genome_bases;  /* concatenated bases resident on this device */
    int64_t hbm_bytes;     /* device memory held by the index image (seeds + device-resident genomes + tables) */
    int64_t seed_bytes;    /* device memory of the packed seed image alone (partition tables + key and value streams) */
    int64_t outlier_seeds; /* seeds kept in the flat 16-byte form (k-mer does not start with its mask's prefix) */
    int32_t key_bits, val_bits, partition_bases; /* packed seed layout: bits per k-mer remainder / value, bases per partition */
    int32_t pad;
} lm_index_info;

/* search.go:631-731 flag defaults */
void lm_options_default(lm_options *opt);

/* Replaces NewIndexSearcher(dir, opt) + SetSeqCompareOptions (lib-index-search.go:237-757, :217): reads info.toml,
 * masks.bin, seeds/chunk_*.bin(.idx), genomes/batch_NNNN/genomes.bin(.idx), genomes.map.bin and builds the HBM image on
 * HIP device `device`.  Limits of this build: at most 65535 masks (the reference's default is 20 000, 40 000 before
 * v0.6.0), genomes of at most 2^28 bases (the reference's own limit, lib-index-build.go:421-425). */
lm_status lm_index_open(const char *dir, const lm_options *opt, int device, lm_index **out);
/* Synthetic genome set + seed index generated directly in HBM (benchmark input; nothing in the reference corresponds to
 * it — an index of real genomes is built with lm_index_builder_* below).  Genome g belongs to family g % families; genomes >= families are
 * mutated copies (substitution rate U(0,max_div), indel shifts at a tenth of that) of the family ancestor.  Honors
 * opt->shard_rank/shard_count.  The seeds come from the pipeline lm_index_builder_* uses (one set of kernels):
 * captures, desert seeds and reversed seeds are the reference's for these genomes, including - for genomes too short to
 * contain every p-base mask prefix, below about 100 kb with 20 000 masks - the rule that a mask without a k-mer of its prefix
 * captures the argmin over all k-mers; earlier builds left such masks without a capture.  k must be 31, masks in
 * [4, 65535] and at most 2 * 4^p (p = floor(log4 masks)), max_desert and seed_dist >= 1: LM_ERR_ARG otherwise. */
typedef struct lm_synth_spec {
    int32_t k;            /* 31 */
    int32_t masks;        /* 20000 (index.go:560) */
    int64_t mask_seed;
    int64_t genomes;      /* genomes in the whole set */
    int32_t genome_len;   /* bases per genome (one contig) */
    int32_t families;
    double max_div;
    int64_t seed;
    int32_t max_desert;   /* 100 (index.go:582) */
    int32_t seed_dist;    /* 50 (index.go:584) */
} lm_synth_spec;
lm_status lm_index_build_synthetic(const lm_synth_spec *spec, const lm_options *opt, int device, lm_index **out);
/* Residency of the 2-bit genomes (residency).  The seed image is always in HBM; the genomes are too when they fit,
 * else - or on request - they live in pinned host memory and a search copies the byte ranges of its chain windows to the
 * device (k_stage_genome_bits).  Rows are the same wherever a genome lives.
 *   LM_GENOMES_DEVICE: every genome in HBM (the open / build fails when the store does not fit);
 *   LM_GENOMES_HOST:   every genome in pinned host memory;
 *   LM_GENOMES_AUTO:   genomes in local order go to HBM while genome_hbm_bytes last (padding counted), the first that does
 *                      not fit and all after it to pinned host memory; a genome is never split.  genome_hbm_bytes = 0: the
 *                      budget is the free device memory beside the seed image minus a scratch floor and a 3-GB reserve.
 * res == NULL (and the plain lm_index_open / lm_index_build_synthetic) = AUTO with budget 0: everything in HBM whenever it fits.
 * LM_GENOME_PLACEMENT=auto|device|host and LM_GENOME_HBM_MB=<n> (measurement only, read at open / build) stand in for a NULL
 * res; a non-NULL res wins.  A pinned allocation the host refuses is LM_ERR_NOMEM; an unknown `genomes` value LM_ERR_OPTION. */
enum { LM_GENOMES_AUTO = 0, LM_GENOMES_DEVICE = 1, LM_GENOMES_HOST = 2 };
typedef struct lm_residency {
    int32_t genomes;            /* LM_GENOMES_* */
    int32_t pad;
    int64_t genome_hbm_bytes;   /* AUTO: device bytes the genome store may take; 0 = derive from free HBM */
} lm_residency;
typedef struct lm_residency_info {
    int64_t genomes_device, genomes_host;
    int64_t genome_bytes_device, genome_bytes_host;   /* 2-bit bytes incl. padding */
    int64_t stage_bytes;        /* device staging buffer(s) currently held for host-resident windows */
} lm_residency_info;
lm_status lm_index_open_ex(const char *dir, const lm_options *opt, const lm_residency *res, int device, lm_index **out);
lm_status lm_index_build_synthetic_ex(const lm_synth_spec *spec, const lm_options *opt, const lm_residency *res, int device, lm_index **out);
lm_status lm_index_get_residency(const lm_index *idx, lm_residency_info *info);
/* ---------------------------------------------------------------------------------------------------------
 * Index building from caller-supplied genomes (what `lexicmap index` does after it has read its FASTA files,
 * lib-index-build.go:880-1407, 1581-1678): an incremental builder - the host streams genomes, every call borrows its
 * arguments only until it returns - whose finish() leaves a handle like lm_index_open's: search, lm_index_mask_seeds,
 * lm_index_fetch, lm_index_save, the genome filter and residency work on it unchanged.
 *   lm_index_builder_add: one input genome.  Its contigs are joined with contig_interval A's; a contig that would take the
 *     concatenation past max_genome starts the next chunk (genome record) of the same genome (:1581-1658), and the chunk list
 *     goes where genomes.chunks.bin goes.  Bases are 2-bit coded by genome/genome.go:1427-1444 (N and most ambiguity codes
 *     become A).  Spacers and runs of >= 5 N are skip regions (lib-gaps.go:38-60): no seed overlaps them.  Record number n
 *     (counted over all accepted records, on every shard) gets the key (n / genome_batch_size) << 17 | n % genome_batch_size.
 *     LM_ERR_ARG, nothing added, builder still usable: no contig, a contig longer than max_genome ("skipping a big genome",
 *     :1601-1610), a record shorter than k or of 2^28 bases or more.  With opt->shard_count > 1 every rank is shown every
 *     genome and keeps those whose first record number % shard_count == shard_rank (the loader's rule).
 *   lm_index_builder_finish: captures (LexicHash, with the masks-without-a-matching-prefix rule), seed-desert filling, reversed
 *     seeds, packed seed image; `res` of _new is honoured as by lm_index_build_synthetic_ex.  The builder is consumed whether
 *     finish succeeds or not; after a failure lm_last_error(NULL) has the text.  LM_ERR_ARG when nothing was added.
 * Not done here (nor by the reference at this point): reading FASTA / gz files, soft-masking, --max-kmer-freq (genomes are
 * ADDED to a resident index by lm_index_builder_extend, resident indexes are joined and subset by
 * lm_index_builder_add_index; joining SHARDS is not done).
 * Only the GENERATED masks are limited: lm_index_builder_new makes its own mask set, and that generator takes k = 31 and puts
 * at most two masks on a p-base prefix (masks <= 2 * 4^p).  lm_index_builder_new_masks builds with the caller's masks - any
 * k in [10, 32], up to 32 masks on a prefix - and _extend, _like and _add_index take whatever set their index carries under
 * the same rule. */
typedef struct lm_build_opt {      /* lm_build_opt_default(): the defaults of `lexicmap index` (index.go:538-619) */
    int32_t k;                     /* 31.  _new (generated masks) and lm_index_build_synthetic: only 31; _new_masks: [10, 32] */
    int32_t masks;                 /* 20000.  _new: [4, 65535] with at most two masks per p-base prefix, p = max(1, floor(log4 masks)):
                                    * 4..8, 16..32, 64..128, 256..512, 1024..2048, 4096..8192, 16384..32768; others: LM_ERR_ARG.
                                    * _new_masks: ignored (its nmasks rules) */
    int64_t mask_seed;             /* 1.  _new_masks: not used to build, written to info.toml as rand-seed */
    int32_t max_desert, seed_dist; /* 100, 50 */
    int32_t contig_interval;       /* 1000 */
    int32_t genome_batch_size;     /* 5000; [1, 2^17] */
    int32_t max_genome;            /* 20000000; <= 0: 2^28 - 1 */
} lm_build_opt;
typedef struct lm_contig {
    const char *id;
    const uint8_t *seq;
    uint32_t len;
} lm_contig;
typedef struct lm_index_builder lm_index_builder;
void lm_build_opt_default(lm_build_opt *o);
/* A builder with a mask set generated here from bo->mask_seed (not lexichash's generator).  Only these generated masks are
 * limited: k == 31 and bo->masks <= 2 * 4^p, else LM_ERR_ARG. */
lm_status lm_index_builder_new(const lm_build_opt *bo, const lm_options *opt, const lm_residency *res, int device, lm_index_builder **out);
/* As lm_index_builder_new, with the caller's mask set (`lexicmap index -M/--mask-file`: the masks `lexicmap utils masks`
 * printed for an existing index, so that the new index can be joined with it).  bo->k is the k of the masks, bo->masks is
 * ignored (nmasks rules), bo->mask_seed is not used to build and is what lm_index_save writes as rand-seed.  The masks are
 * copied before the call returns.  Accepted: k in [10, 32]; nmasks in [4, 65535]; masks strictly ascending and below 4^k;
 * with p = max(floor(log4 nmasks), 1) every p-base prefix has at least one mask and none more than 32.  Anything else is
 * LM_ERR_ARG and lm_last_error(NULL) names the first offending mask (0-based), the first prefix without a mask, or the prefix
 * with too many and its count.  The option checks of _new apply unchanged (min_prefix against k and p + anchor_prefix, ...).
 * A set in which every prefix has one mask or two gives the very index _new gives for the same masks.  add, add_index,
 * finish, free, last_error, sharding by opt->shard_count, residency, save, mask_seeds, seed_positions and seed_distances
 * work as with _new. */
lm_status lm_index_builder_new_masks(const lm_build_opt *bo, const uint64_t *masks, size_t nmasks, const lm_options *opt,
                                     const lm_residency *res, int device, lm_index_builder **out);
lm_status lm_index_builder_add(lm_index_builder *b, const char *genome_id, const lm_contig *contigs, size_t ncontigs);
lm_status lm_index_builder_finish(lm_index_builder *b, lm_index **out); /* consumes b on success and on failure */
void lm_index_builder_free(lm_index_builder *b);                        /* abandon */
const char *lm_index_builder_last_error(const lm_index_builder *b);
/* A builder that continues `base`.  finish() gives a NEW handle holding base's genomes followed by the added ones: what one
 * lm_index_builder_* build of all of them, in that order, with base's masks would have given (the same lists, keys, store
 * and saved files).  Only the added records are captured; base's seeds are decoded from its image and packed again.
 *   The device, the lm_options (shard_rank / shard_count and total_bases_override among them) and the masks are base's.
 *   bo == NULL: k, masks, contig_interval, genome_batch_size, max_desert and seed_dist are what the handle carries (an opened
 *     index: what its info.toml says), max_genome its default.  A non-NULL bo must agree with base in k, masks,
 *     contig_interval and genome_batch_size (LM_ERR_ARG, the text names the field); its mask_seed is IGNORED, because the
 *     masks are base's; its max_desert, seed_dist and max_genome apply to the added genomes.
 *   Record numbers continue from base's record count over all shards; a shard keeps the genomes whose first record number
 *     % shard_count == shard_rank.  Every batch of base but the last must hold exactly genome_batch_size records: a base
 *     with irregular batches (an index of the reference with split genomes is one) is refused with LM_ERR_ARG.
 *   add / finish / free / last_error work as on a builder of _new; finish with nothing added is LM_ERR_ARG.  base is only
 *     read: it stays open, unchanged and searchable, the caller closes it - but it must stay open until finish or free has
 *     returned, and finish holds base's lock while it reads.  The new handle starts without a genome filter.
 *   base's image, the new image and the seed staging arrays are on the device together; LM_ERR_NOMEM (base intact, the
 *     builder consumed) when they do not fit. */
lm_status lm_index_builder_extend(lm_index *base, const lm_build_opt *bo, const lm_residency *res, lm_index_builder **out);
/* Appends the genome records of a resident index to the builder, in src's record order, numbered on from the builder's
 * record count: what _add of those genomes, in that order, would have appended - without capturing them again.  finish()
 * copies their 2-bit records, decodes their seeds from src's image, gives them the new keys and packs them with the rest.
 * keep == NULL: all records.  Otherwise keep[0..nkeep) are record keys of src (batch << 17 | index, as
 * lm_index_set_genome_filter takes them); only those records are appended, still in src's order.
 *   _add and _add_index may be called in any order and any number of times on a builder of _new, _extend or _like: join
 *     (_extend(A), _add_index(B)), N-way join, subset (_like(A), _add_index(A, keep)), and genomes added in between.
 *   Preconditions, each refused with LM_ERR_ARG and a text (lm_index_builder_last_error) that names what differs; nothing is
 *     added and the builder stays usable: src and the builder agree in k, in contig_interval, in the number of masks and in
 *     the mask VALUES (two sets of as many masks from different seeds are different masks); both are on the same device; both
 *     are unsharded (shard_count == 1: joining shards would move records between ranks); src is not the builder's base and
 *     was not added to this builder before.
 *   Keep list, LM_ERR_ARG likewise: a key that is no record of src; a key given twice; a genome that was split into several
 *     records (genomes.chunks.bin) named with some of its records but not all; an empty selection (keep != NULL, nkeep == 0).
 *   src's batch layout does not matter, every record is renumbered: an index with irregular batches, which _extend refuses
 *     as a base, is a legal source.
 *   Every appended record is a copy of src's (genome id, contig ids and sizes, genome size, length) under its new key; chunk
 *     lists keep their shape under new list numbers; the input-genome count grows by the genomes appended (a split genome
 *     counts once), the input bases by their genome sizes.  lm_index_get_info and lm_index_save of the result equal those of
 *     one build of the same genomes in the same order.  max-seed-dist and seed-dist-in-desert of the result are the
 *     builder's: those of a source are NOT checked, its deserts were filled when it was built.
 *   src is only read.  It must stay open until finish or free has returned; finish holds the locks of the base and of every
 *     source while it reads (taken in the order of the handles' addresses).  Sources stay open, unchanged and searchable; a
 *     source's genome filter is not carried.
 *   The sources, the new store, the new image and the seed staging arrays are on the device together; LM_ERR_NOMEM (sources
 *     intact, the builder consumed, the text says so) when they do not fit.  Sources are not released as they are consumed. */
lm_status lm_index_builder_add_index(lm_index_builder *b, lm_index *src, const uint64_t *keep, size_t nkeep);
/* An empty builder with the masks, lm_options, device and build settings of `model` (nothing of its genomes): what _extend
 * gives, minus the base.  bo / res as in _extend, with the same refusals for a bo that disagrees with model in k, masks,
 * contig_interval or genome_batch_size; model's batches need not be regular, since nothing is continued.  model is only
 * read, and only during this call.  finish with nothing added stays LM_ERR_ARG. */
lm_status lm_index_builder_like(const lm_index *model, const lm_build_opt *bo, const lm_residency *res, lm_index_builder **out);
/* bases [start, start+len) of local genome `local_genome` as ASCII (used to derive synthetic queries) */
lm_status lm_index_fetch(lm_index *idx, int64_t local_genome, int64_t start, int64_t len, uint8_t *out);
/* Writes the resident (unsharded) index to `dir`: info.toml, seeds/chunk_NNN.bin (+ .idx, kv/kv-data.go:126-602) in at most
 * `chunks` files, genomes/batch_NNNN/genomes.bin (+ .idx, genome/genome.go:217-357), genomes.map.bin and genomes.chunks.bin in the reference's
 * on-disk format; masks.bin in THIS build's own layout (LMMASKS1: lexichash's file layout is not in the reference tree), so
 * lm_index_open and the oracle read the result back, the reference's Go binary does not.  info.toml carries the format
 * version, k, masks, chunk files, partitions, genome counts, input bases and the contig interval; the build-time settings it
 * does not know (rand-seed, the seed-distance settings, soft-masking, max-kmer-freq) are written as the reference's defaults
 * and are not read by a search.  Used to time the loader at benchmark scale on GPU-built sets.
 * genomes.chunks.bin (the chunk lists of genomes split at --max-genome, lib-index-build.go:1787-1808) is written too - empty
 * when no genome was split.  A shard (shard_count > 1) is refused. */
lm_status lm_index_save(lm_index *idx, const char *dir, int chunks);
/* Replaces (*Index).Close (lib-index-search.go:760) */
void lm_index_close(lm_index *idx);
lm_status lm_index_get_info(const lm_index *idx, lm_index_info *info);
/* masks of the index (lexichash.LexicHash.Masks), borrowed until close */
const uint64_t *lm_index_masks(const lm_index *idx);
/* (k-mer, value) pairs stored under one mask (normal seeds, then reversed seeds; each part ascending by k-mer), values
 * in the reference layout batch:17|genome:17|pos:28|rc:1|reversed:1: kv.Reader.ReadDataOfAMaskAsList
 * (kv/kv-reader.go:762), what `lexicmap utils kmers --mask` prints (kmers.go:101-180). Call with cap = 0 (or both arrays
 * NULL) for the count; 0 < cap < count returns LM_ERR_ARG with *n = count and writes nothing. */
lm_status lm_index_mask_seeds(lm_index *idx, int32_t mask, uint64_t *kmers, uint64_t *vals, size_t cap, size_t *n);
/* Where the seeds of genome records are, from the resident image: what `lexicmap utils seed-pos` reads from
 * seed_positions.bin (seed-pos.go), a file a resident index does not have.  One device pass over the packed values of the
 * forward lists (the reversed lists repeat the same positions), one radix sort, one segmentation; the genome bytes are not
 * read, so it works wherever they live, on built, opened, extended, joined and subset handles.
 *   keys[0..nkeys): record keys (batch << 17 | index); keys == NULL with nkeys == 0: every record of this handle in record
 *     order; keys != NULL with nkeys == 0: no record, an empty result.  Record slot s of the result is keys[s] (or the
 *     handle's s-th record).
 *   lm_seedpos_get: returns the number of record slots n; keys[n], off[n + 1], locs[off[n]]: the position list of slot s is
 *     locs[off[s] .. off[s + 1]), loc = pos << 1 | strand (the reference's value without genome key and reverse bit:
 *     (value >> 1) & (2^29 - 1)), ascending as uint32; a position captured by two masks is there twice
 *     (lib-index-build.go:1066-1072, 1409-1417).  Any of the three pointers may be NULL.  Valid until lm_seedpos_free.
 * LM_ERR_ARG, text in lm_last_error(idx), handle still usable: a key that is no record of this handle (a sharded handle
 * answers for its own records: the text says when the key is a record of another shard), a key given twice, keys == NULL
 * with nkeys > 0.  LM_ERR_NOMEM (text says what had to fit) when the 20 B per selected forward seed - two 8-byte arrays of
 * sort keys and the 4-byte position list - or the radix sort's scratch do not fit beside the index. */
typedef struct lm_seedpos lm_seedpos;
lm_status lm_index_seed_positions(lm_index *idx, const uint64_t *keys, size_t nkeys, lm_seedpos **out);
size_t lm_seedpos_get(const lm_seedpos *sp, const uint64_t **keys, const int64_t **off, const uint32_t **locs);
void lm_seedpos_free(lm_seedpos *sp);
/* The distances between consecutive seeds of the selected records, computed on the device from the sorted position lists
 * (the rule: lexicmap_amd/csrc/lm_seed_dist.h; seed-pos.go:385-457 without its flag bit).  A record's
 * contigs start at s_0 = 0, s_{c+1} = s_c + len_c + contig_interval; position p = loc >> 1 belongs to the last contig with
 * s_c <= p; the first position of a contig has dist = p - s_c, every other dist = p - the position before; a contig without
 * seeds contributes nothing; a run of N inside a contig counts as sequence.  A position is REPORTED when dist >= min_dist.
 *   records: one per slot, whatever min_dist is - seeds (entries of the position list), the largest dist and the first
 *     position that has it (both 0 without seeds), contigs and how many of them hold no seed.
 *   hist: hist_bins counters of width hist_width over the reported positions of all selected records (what seed-pos plots),
 *     the last counter taking everything beyond; hist_bins == 0: none.  At most 4096 counters.
 *   rows: the reported positions, records in selection order, positions ascending within a record: what
 *     `utils seed-pos -D min_dist` prints (pos and pos_in_contig are 0-based here, the tool prints them + 1).
 * opt == NULL: {0, 0, 0}.  LM_ERR_ARG beyond the cases of lm_index_seed_positions: hist_bins > 0 with hist_width < 1,
 * hist_bins > 4096.  The accessors return the element count; results are valid until lm_seed_dist_free. */
typedef struct lm_seed_dist_opt {
    uint32_t min_dist;   /* -D/--min-dist of seed-pos */
    uint32_t hist_bins;
    uint32_t hist_width;
    uint32_t pad;
} lm_seed_dist_opt;
typedef struct lm_seed_dist_rec {
    uint64_t key;
    int64_t seeds;
    uint32_t max_dist, max_dist_pos;
    int32_t contigs, contigs_without_seeds;
} lm_seed_dist_rec;
typedef struct lm_seed_dist_row {
    uint32_t record;         /* slot in the selection */
    uint32_t contig;         /* index of the contig in the record */
    uint32_t pos;            /* 0-based in the record's concatenation */
    uint32_t pos_in_contig;  /* pos - s_c */
    uint32_t strand;         /* 1: the k-mer was captured on the reverse strand */
    uint32_t dist;
} lm_seed_dist_row;
typedef struct lm_seed_dist lm_seed_dist;
lm_status lm_index_seed_distances(lm_index *idx, const uint64_t *keys, size_t nkeys, const lm_seed_dist_opt *opt, lm_seed_dist **out);
size_t lm_seed_dist_records(const lm_seed_dist *sd, const lm_seed_dist_rec **recs);
size_t lm_seed_dist_hist(const lm_seed_dist *sd, const uint64_t **hist);
size_t lm_seed_dist_rows(const lm_seed_dist *sd, const lm_seed_dist_row **rows);
void lm_seed_dist_free(lm_seed_dist *sd);
/* ---------------------------------------------------------------------------------------------------------
 * Genome screening: which genomes of the index are closest to this assembly?  The first stage of `lexicmap genome search`,
 * what -S/--only-genome-screening prints (GSearchScreen, lib-index-search-genome.go:114-543), for a batch of query genomes
 * in one call, on the device (lexicmap_amd/csrc/lm_screen.hip; the rule and its deterministic choices: DESIGN.md section 11).
 *   Query genome (search-genome-util.go:129-244): contigs pass the 2-bit base table (N and n become A BEFORE any gap is
 *     looked for: a run of N is no skip region here, unlike in the builder) and are joined by k skipped bases; the skip
 *     regions are exactly those spacers.  A query of fewer than k bases gives no rows.
 *   Windows (:150-207): step = len / (windows + 1); window i is [i * step, i * step + 2 * step), the last one runs to len,
 *     windows == 1 is the whole sequence.  Every window is masked on its own with the missing-prefix rule and - the
 *     reference's behaviour, :180 - with the UNSHIFTED region list of the whole sequence.  Captures that are 0, CCC..,
 *     GGG.., TTT.. or DUST > 50 are dropped; per mask the k-mers of all windows are de-duplicated.
 *   Lookup (:371, kv-searcher2.go:326-549): every k-mer of mask m is range-searched in the forward list of m over
 *     [kmer & ~low, kmer | low], low = 4^(k - min_prefix) - 1; every stored VALUE in range counts once with
 *     Len = LCP(query k-mer, stored k-mer).  Values of genomes outside lm_index_set_genome_filter's whitelist count nowhere.
 *     As in the reference, whose search starts from an anchor index in which a later run of k-mers with the same anchor bases
 *     hides an earlier one (kv-reader.go:762-1021), a lookup returns nothing when the mask's list holds such a later run; only
 *     lists with k-mers of other prefixes than their mask's (captures of tiny genomes) have one.
 *   Per subject record (:316-341): score = sum of Len; with details, per mask Hits (saturating at 255) and Longest, and
 *     from them hit_masks = #masks hit, hit_kmers = sum of Hits, score2 = sum of Longest, prefixes = Longest of the hit masks,
 *     descending (search-genome.go:554-591).  details == 0: those fields are 0 and there are no prefixes.
 *   Records of one split genome (:423-496) are one row: score summed over its hit records, the hit records' keys
 *     ascending, details of the hit record with the LOWEST key (the reference takes whichever a Go map yields first).
 *   Rows of a query (:498-509): score descending, ties by ascending lowest key (the reference: an unstable sort), cut to
 *     top_n (0: all).  Rows are grouped by query in input order.  A sharded handle answers for its own records
 *     (lm_index_screen_add_structure below makes its rows the unsharded index's rows for them).
 * LM_ERR_ARG, text in lm_last_error(idx), handle still usable: windows < 1, nq > 0 with queries == NULL, a query without
 * contigs, a query of 2^28 bases or more.  LM_ERR_OPTION: min_prefix outside [mask_prefix + anchor_prefix, k].
 * LM_ERR_NOMEM (the text says what had to fit) when the (query, record, mask, Len) tuples of ONE mask do not fit beside
 * the index: the tuples of a batch pass through the device in pieces of whole masks cut from a counting pass.
 * LM_SCREEN_PIECE_TUPLES=<n> (tests and measurement only, read at call time) caps a piece at n tuples (or one mask's, when
 * that is more), so that the multi-piece path runs on small input; no result depends on it.  opt == NULL: the defaults. */
typedef struct lm_screen_opt {     /* lm_screen_opt_default(): the flag defaults of search-genome.go:729-739 */
    int32_t min_prefix;            /* 21 */
    int32_t windows;               /* 1 */
    int32_t top_n;                 /* 10; 0 keeps all */
    int32_t details;               /* 0 */
} lm_screen_opt;
typedef struct lm_genome_query {
    const char *id;                /* not read by the screen: the printer's first column */
    const lm_contig *contigs;
    size_t ncontigs;
} lm_genome_query;
typedef struct lm_screen_row {
    uint32_t query;                /* index into the batch */
    uint32_t nkeys;                /* hit records of the genome: keys[keys_off .. keys_off + nkeys), ascending */
    uint64_t score;
    uint64_t batch_genome;         /* the lowest of those keys */
    const char *genome_id;         /* borrowed from the index, valid until lm_index_close */
    uint64_t keys_off;
    uint64_t score2;
    uint32_t hit_masks;            /* = number of prefixes: prefixes[prefixes_off .. prefixes_off + hit_masks) */
    uint32_t pad;
    uint64_t hit_kmers;
    uint64_t prefixes_off;
} lm_screen_row;
typedef struct lm_screen_stats {   /* measured work of the call */
    int64_t query_bases, windows, lookups, tuples, pieces; /* lookups: de-duplicated k-mers a list could match */
    double ms_capture, ms_lookup, ms_reduce, ms_total;
} lm_screen_stats;
typedef struct lm_screen lm_screen;
void lm_screen_opt_default(lm_screen_opt *o);
lm_status lm_index_screen_genomes(lm_index *idx, const lm_genome_query *queries, size_t nq, const lm_screen_opt *opt, lm_screen **out);
/* the accessors return the element count; any pointer may be NULL; valid until lm_screen_free */
size_t lm_screen_rows(const lm_screen *s, const lm_screen_row **rows);
size_t lm_screen_keys(const lm_screen *s, const uint64_t **keys);
size_t lm_screen_prefixes(const lm_screen *s, const uint8_t **prefixes);
void lm_screen_get_stats(const lm_screen *s, lm_screen_stats *stats);
void lm_screen_free(lm_screen *s);
/* Screening with shards.  The reference's anchor index (above) is a property of a mask's WHOLE list, and a shard holds the seeds
 * of its own records only: left alone, a shard misses the hiding runs of other shards' records and its sums can exceed what the
 * unsharded index gives for the same records.  lm_index_screen_structure exports what the rule reads of this handle's lists -
 * per list a bitmap of the occupied partitions and the outlier k-mers, no values: 64 bits per 64 partitions and 8 B per outlier
 * (*blob, *bytes; released with lm_free) - and lm_index_screen_add_structure adds another shard's to this handle.  Once every
 * rank has added the structure of every other rank (the host carries the blobs, once per index), the rows of a rank are the
 * unsharded index's rows for its records, and the union of all ranks' rows at top_n = 0 is the unsharded result.  blob == NULL
 * or bytes == 0: back to the handle's own lists.  LM_ERR_ARG, the handle as it was: a blob of an index with other k, masks or
 * partitions, a broken blob (wrong length, outlier offsets or k-mers of a list not ascending), a partition index of more than 6
 * bases.  LM_ERR_NOMEM / LM_ERR_HIP while the union is put on the device: the handle is back to its own lists, never left with
 * half a union.  The blob needs no alignment (it is copied out).  Its layout, all little-endian: uint64 magic; int32 k, masks,
 * mask prefix, partition bases, W = words per list bitmap, 0; int64 outliers; uint64 bitmaps[2 * masks][W] (list 2 * mask +
 * direction); int64 offsets[2 * masks + 1]; uint64 k-mers[outliers], ascending within a list.  The handle keeps the union on the
 * host and on the device: 16 B per list and W word, 20 MB each at 20 000 masks, plus 8 B per outlier k-mer.
 * These two calls go beyond what `lexicmap genome search` has: the reference has no shards. */
lm_status lm_index_screen_structure(lm_index *idx, void **blob, size_t *bytes);
lm_status lm_index_screen_add_structure(lm_index *idx, const void *blob, size_t bytes);
/* One line of -S (search-genome.go:577-590; no newline): query id, subject id, minPrefix, fracMasks = hit_masks / masks,
 * nMasks, sumPrefix = score2, avgPrefix = score2 / hit_masks as "%s\t%s\t%d\t%.4f\t%d\t%d\t%.2f", and with `extra` a tab and
 * the comma-joined prefixes (`prefixes` = the array lm_screen_prefixes gives).  Returns the length that was / would be written. */
int lm_format_screen_row(const lm_screen_row *row, const uint8_t *prefixes, const char *query_id, int min_prefix, int masks,
                         int extra, char *buf, size_t buflen);
/* the header line of -S (search-genome.go:482-486), no newline */
const char *lm_screen_header(int extra);
/* ---------------------------------------------------------------------------------------------------------
 * Similar genome pairs: which records of this index are near-duplicates of each other?  What `lexicmap genome pair`
 * computes with -s 0 (lexicmap/cmd/pair.go), on the device from the packed image alone (lexicmap_amd/csrc/lm_pairs.hip; the
 * rule, the passes and their memory: DESIGN.md section 11).  The genome bytes are not read, so it works wherever they live,
 * on built, opened, extended, joined and subset handles.
 *   Masks (-m, :162-184): masks == 0 takes every mask; otherwise the FIRST mask (index order) of every distinct q-base prefix,
 *     q = log4(masks).  total_masks = the number of masks taken (the distinct prefixes present, not necessarily `masks`).
 *   Seeds: the forward seeds of a taken mask (both strands).  Two seeds of one mask match when their k-mers share at least
 *     min_prefix (-p) leading bases; per mask and unordered pair of DIFFERENT records the largest common prefix over all
 *     matching seed pairs counts (:903-931, :943-962).  n_masks = masks in which the pair matched, sum_prefix = the sum of
 *     those per-mask maxima (:286-291).
 *   Rows (:704, :995-1004): pairs with n_masks >= required = (int)(min_mask_fraction * total_masks) (-f), ordered by n_masks
 *     descending, sum_prefix descending, (key1, key2) ascending; key1 < key2.  A split genome's records are separate
 *     "genomes" here, as in the reference.
 *   -s/--prob-threshold is always 0: the reference's probabilistic pruning depends on the order in which its workers deliver
 *     masks and is not reproduced.  A pair is dropped early only when n_masks so far + masks not yet processed < required,
 *     which changes no row.
 *   min_prefix must lie in [mask_prefix + anchor_prefix, k]: a group of matching seeds then lies inside one partition of the
 *     packed list or inside the outlier list.  The shorter prefixes the reference accepts are not supported.
 *   keys / nkeys as in lm_index_seed_positions: NULL = every record of the handle; otherwise only seeds of the given records
 *     take part (pairs among a subset of a big index); keys != NULL with nkeys == 0: no rows.  The genome whitelist of
 *     lm_index_set_genome_filter is NOT consulted.
 * LM_ERR_OPTION, text in lm_last_error(idx), handle still usable: min_prefix out of range; masks neither 0 nor a power of 4
 * >= 64, or above the index's mask count; min_mask_fraction negative or NaN.  LM_ERR_ARG: a key that is no record, a key given
 * twice, keys == NULL with nkeys > 0, a sharded handle (a shard cannot see the pairs across shards).  LM_ERR_NOMEM (the text
 * says what had to fit): the 36 B per forward seed of the taken masks and records, the 25 B per candidate seed pair of ONE
 * mask (the tuples pass through the device in pieces of whole masks), or the 32 B per row of the pair table, which stays on
 * the device until the end.  LM_PAIR_PIECE_TUPLES=<n> (tests and measurement only, read at call time) caps a piece at n tuples
 * (or one mask's, when that is more); no result depends on it.  opt == NULL: the defaults. */
typedef struct lm_pair_opt {       /* lm_pair_opt_default(): the flag defaults of pair.go */
    int32_t min_prefix;            /* 21 */
    int32_t masks;                 /* 1024 */
    double min_mask_fraction;      /* 0.25 */
} lm_pair_opt;
typedef struct lm_pair_row {
    uint64_t key1, key2;           /* record keys, key1 < key2 */
    const char *genome1, *genome2; /* borrowed from the index, valid until lm_index_close */
    uint32_t n_masks, sum_prefix;
} lm_pair_row;
typedef struct lm_pair_stats {     /* measured work of the call */
    int64_t total_masks, required, entries, tuples, pieces, pairs_seen, rows; /* entries: seeds that took part; pairs_seen: distinct pairs that entered the table */
    double ms_entries, ms_emit, ms_reduce, ms_total;
} lm_pair_stats;
typedef struct lm_pairs lm_pairs;
void lm_pair_opt_default(lm_pair_opt *o);
lm_status lm_index_genome_pairs(lm_index *idx, const uint64_t *keys, size_t nkeys, const lm_pair_opt *opt, lm_pairs **out);
/* returns the row count; rows may be NULL; valid until lm_pairs_free */
size_t lm_pairs_rows(const lm_pairs *p, const lm_pair_row **rows);
void lm_pairs_get_stats(const lm_pairs *p, lm_pair_stats *s);
void lm_pairs_free(lm_pairs *p);
/* One line of `lexicmap genome pair` (pair.go:730; no newline): genome1, genome2, minPrefix, fracMasks = n_masks /
 * total_masks, nMasks, sumPrefix, avgPrefix as "%s\t%s\t%d\t%.4f\t%d\t%d\t%.2f".  Returns the length that was / would be written. */
int lm_format_pair_row(const lm_pair_row *r, int min_prefix, int total_masks, char *buf, size_t cap);
/* its header line (pair.go:721), no newline */
const char *lm_pair_header(void);
/* Pairs across the shards of a sharded index ("Pairs across shards").  Shards
 * partition records, not masks: every shard holds every mask's seeds of its own records, and the mask selection and `required`
 * depend on the mask set alone.  So a pair can be evaluated wholly on one rank once that rank has the forward seeds of the
 * other record's shard.  Every rank exports its seeds once (lm_index_pair_seeds); rank r receives the blobs of the ranks
 * s < r - the host carries them, the library moves nothing - and calls lm_index_genome_pairs_across; rank 0 merges the
 * ranks' rows (lm_pairs_merge).  The merged rows are the unsharded index's rows, row for row.  These calls go beyond what
 * `lexicmap genome pair` has: the reference has no shards.
 *
 * lm_index_pair_seeds: the forward seeds of the masks taken by opt->masks (the rule above; min_prefix and min_mask_fraction
 * are not read) of the records keys / nkeys selects (as above), of a sharded or an unsharded handle, as (k-mer, record) in
 * list order per mask: packed list, then outliers.  *blob / *bytes, released with lm_free.  A handle or a selection without
 * records gives a valid blob without records.  The blob needs no alignment; its layout, all little-endian: uint64 magic;
 * int32 k, masks of the index, opt->masks, total_masks = masks taken; uint64 fingerprint of the mask values; int64 records,
 * entries, id_bytes; uint64 keys[records], ascending; uint16 id_len[records]; char ids[id_bytes] (the genome ids back to back,
 * no terminators); int64 offsets[total_masks + 1] (the first entry of every taken mask); uint64 kmers[entries]; uint32
 * record[entries] (index into keys).  12 B per seed, 10 B and its id per record.  LM_ERR_OPTION / LM_ERR_ARG as
 * lm_index_genome_pairs for masks and keys; a genome id of more than 65535 bytes is LM_ERR_ARG.
 *
 * lm_index_genome_pairs_across: the rows - the rule, the order and the options of lm_index_genome_pairs, unchanged, key1 <
 * key2 over the global record keys - of the pairs among the handle's own selected records and of the pairs between an own
 * record and a record of any blob.  Two blob records are never a row.  The handle may be a shard or unsharded; nblobs == 0
 * gives the pairs within the handle, which lm_index_genome_pairs refuses to give for a shard.  genome1 / genome2 of an own
 * record are borrowed from the index as above; those of a blob record point into storage the RESULT owns and are valid until
 * lm_pairs_free.  stats.entries counts own and blob seeds, stats.tuples the candidate seed pairs emitted: every pair of seeds
 * of a group is emitted on exactly one rank.  LM_ERR_OPTION as lm_index_genome_pairs.  LM_ERR_ARG, the text naming the blob
 * number and what differs, the handle as it was: a blob of another k, mask count or mask values; a blob exported with
 * another opt->masks; a broken blob (length, offsets not monotone, a record index out of range, keys not ascending); a record
 * key that is also an own record or occurs in two blobs; blobs == NULL with nblobs > 0; more than 2^29 records in the union.
 * LM_ERR_NOMEM as above, the blob seeds counted in: with blob seeds the entries are sorted on the device, 32 B per seed
 * while sorted, 49 B while the groups are scanned, 32 B afterwards.
 *
 * lm_pairs_from_rows: rows that reached this process some other way (a rank's rows over the wire) as a result of their
 * own; the rows and their names are copied, stats may be NULL.  lm_pairs_merge: a host k-way merge of n results by the
 * rule's order.  Every name is COPIED into the merged result, which does not depend on the parts or on any index afterwards.
 * Its stats are the parts' sums (total_masks and required: the largest).  LM_ERR_ARG: a part that is NULL or not in the
 * rule's order, a pair that occurs twice - the ranks did not follow the s < r scheme.  Neither call takes a handle: the text
 * of a refusal is lm_last_error(NULL). */
lm_status lm_index_pair_seeds(lm_index *idx, const uint64_t *keys, size_t nkeys, const lm_pair_opt *opt, void **blob, size_t *bytes);
lm_status lm_index_genome_pairs_across(lm_index *idx, const uint64_t *keys, size_t nkeys, const void *const *blobs, const size_t *blob_bytes,
                                       size_t nblobs, const lm_pair_opt *opt, lm_pairs **out);
lm_status lm_pairs_from_rows(const lm_pair_row *rows, size_t n, const lm_pair_stats *stats, lm_pairs **out);
lm_status lm_pairs_merge(const lm_pairs *const *parts, size_t n, lm_pairs **out);
/* text of the last error on this handle, or of the last failed lm_index_open when idx == NULL */
const char *lm_last_error(const lm_index *idx);

/* ---------------------------------------------------------------------------------------------------------
 * Whole-path entry point: replaces the per-query goroutines calling (*Index).Search (search.go:548-608,
 * lib-index-search.go:1191-2940) with one batched call. */
typedef struct lm_query {
    const uint8_t *seq; /* upper-case bases (the host upper-cases, search.go:580-587) */
    uint32_t len;
} lm_query;

/* One HSP row = what the TSV printer consumes (search.go:468-523); coordinates 0-based inclusive. */
typedef struct lm_hsp {
    uint32_t query;        /* index into the batch */
    uint32_t hits;         /* number of subject genomes of this query ("hits" column) */
    uint64_t batch_genome; /* batch<<17 | genome index (key of genomes.map.bin) */
    double qcov_genome;    /* qcovGnm */
    int32_t cls, hsp;      /* 1-based counters as printed */
    int32_t seq_idx, nseqs, seq_len, nchunks, chunk_idx;
    int32_t rc;            /* subject strand '-' */
    double qcov_hsp;
    int32_t aligned_length;
    double pident;
    int32_t gaps;
    int32_t qbegin, qend, tbegin, tend;
    double evalue;
    int32_t bitscore, score, matched_bases;
    const char *genome_id, *seq_id;          /* borrowed from the index, valid until lm_index_close */
    const char *cigar, *qseq, *sseq, *align; /* only with output_seq; owned by the result batch */
} lm_hsp;

typedef struct lm_stage_stats { /* measured work per batch (H, A, C ...) */
    int64_t query_bases, query_kmers;
    int64_t seed_lookups;      /* (query,mask,direction) probes issued */
    int64_t seed_values;       /* H: seed values returned */
    int64_t anchors_raw;       /* anchors assembled (values x query locations) */
    int64_t genome_pairs;      /* (query,genome) pairs chained */
    int64_t anchors_cleared;   /* A: anchors after de-duplication */
    int64_t chains;            /* C: chains sent to alignment */
    int64_t window_bases;      /* sum of target window lengths */
    int64_t pa_anchors;        /* pseudo-alignment anchors EMITTED: without those nested in the anchor of the neighbouring
                                  window position, which ClearSubstrPairs would drop (LM_PA_DROP_NESTED=0: every anchor) */
    int64_t hsps_aligned;      /* WFA problems */
    int64_t wfa_retries;
    int64_t rows;              /* HSP rows emitted */
    int64_t aligned_bases;     /* sum of alenHSP over emitted rows */
    double ms_mask, ms_lookup, ms_chain, ms_window, ms_pseudo, ms_glue, ms_extend_wfa, ms_finalize, ms_total;
} lm_stage_stats;

typedef struct lm_result lm_result;

/* queries resident in HBM (so that a timed region can exclude the PCIe upload) */
typedef struct lm_qbatch lm_qbatch;
lm_status lm_qbatch_upload(lm_index *idx, const lm_query *queries, size_t nq, lm_qbatch **out);
void lm_qbatch_free(lm_qbatch *qb);
lm_status lm_search_resident(lm_index *idx, lm_qbatch *qb, lm_result **out);
/* = upload + search_resident */
lm_status lm_search_batch(lm_index *idx, const lm_query *queries, size_t nq, lm_result **out);
size_t lm_result_rows(const lm_result *res, const lm_hsp **rows); /* rows grouped by query, in output order */
void lm_result_stats(const lm_result *res, lm_stage_stats *stats);
void lm_result_free(lm_result *res); /* RecycleSearchResults, lib-index-search.go:1170 */
/* search.go:468-523: one TSV line (no newline); returns the length that was/would be written */
int lm_format_row(const lm_hsp *row, const char *query_id, uint32_t qlen, int more_columns, char *buf, size_t buflen);
/* the same line with the printer's two switches (search.go:483-520): LM_ROW_ALL = -a/--all (CIGAR, qseq, sseq, align
 * columns), LM_ROW_SSEQ_IDX = --show-sseq-idx (sseqid as c<chunk>/<chunks>:s<seq>/<seqs>:<id>, :483-494) */
#define LM_ROW_ALL 1
#define LM_ROW_SSEQ_IDX 2
int lm_format_row_ex(const lm_hsp *row, const char *query_id, uint32_t qlen, int flags, char *buf, size_t buflen);
/* The printer's loop over a batch (search.go:468-523; one writer goroutine in the reference): every row as lm_format_row_ex
 * writes it, a newline after each, in row order, formatted by the host threads into ONE buffer (*text, *len bytes, released
 * with lm_free).  query_ids / query_lens: the id and length of batch query i at [i], nq of them (rows[].query indexes them). */
lm_status lm_format_rows(const lm_hsp *rows, size_t n, const char *const *query_ids, const uint32_t *query_lens, size_t nq,
                         int flags, char **text, size_t *len);
/* the header line of the TSV (search.go:426-430), no newline; more_columns as in lm_format_row */
const char *lm_tsv_header(int more_columns);

/* ---------------------------------------------------------------------------------------------------------
 * Subject subsequences and flanks: the bases around the hits of a search, or of any region of a record, from the resident
 * 2-bit genomes in one batched device pass.  What `lexicmap utils subseq` and `lexicmap utils genome-seqs` print
 * (lexicmap/cmd/subseq.go, genome-seqs.go; genome/genome.go SubSeq, SubSeq2), with the rule, the passes and their memory in
 * DESIGN.md section 11 (lexicmap_amd/csrc/lm_subseq_plan.h, lm_subseq.hip).
 *   A region names a record by key (batch << 17 | index), or with key == LM_REGION_BY_NAME by genome_id: the genome's records
 *     are tried in chunk order and the first one that holds the contig id answers (subseq.go:403-423).
 *   The contig: seq_id (non-empty) by id; else seq_idx >= 0 by number (what lm_hsp carries; with a genome id: of the genome's
 *     first record); else (seq_idx < 0) begin / end are concatenated coordinates of the record (-c/--concatenated-positions).
 *   begin <= end are 1-based and inclusive; rc != 0 is the '-' strand: the reverse complement of the same bases, begin / end
 *     stay forward coordinates.  upstream / downstream (-U / -D) extend the region and swap on the '-' strand; the start is
 *     clamped to 1, the end to the contig (to the record in concatenated coordinates): a flank never runs into the spacer
 *     between two contigs.  A region that begins behind its contig's end is answered with no bases.  N is stored as A.
 *   Status per region: LM_SUBSEQ_NO_GENOME (no such key / genome id), LM_SUBSEQ_NO_SEQ (the contig is in none of the genome's
 *     records, a seq_idx beyond the record, or a contig id that occurs twice in one record - name such a contig by seq_idx),
 *     LM_SUBSEQ_OUT_OF_RANGE (concatenated coordinates that begin behind the record's end), LM_SUBSEQ_NOT_LOCAL (a sharded
 *     handle answers for its own records; regions by genome id see the shard's own genomes only).
 *   ignore_errors == 0 (the tool without -e): the first region with a status other than OK makes the call return LM_ERR_ARG,
 *     lm_last_error names the region and what failed, nothing is returned.  ignore_errors != 0 (-e): such regions carry their
 *     status and no bases, the others are answered.  begin < 1, end < begin and negative flanks are LM_ERR_ARG in either mode,
 *     and so is a region of 2^31 bases or more or one whose first base lies behind base 2^32 of its record.
 *   The result: one lm_subseq_info per region, in region order, and ONE blob of ASCII bases (pinned host memory): region i's
 *     bases are blob[off, off + len); off is a multiple of 16, the bytes between two regions are zero.  begin / end are the
 *     extracted range as the tool prints it.  The blob passes through the device in pieces of LM_SUBSEQ_PIECE_BYTES (read at
 *     call time; tests and measurement), by default 256 MB or what the scratch arena can give; no result depends on it.
 * The genome whitelist of lm_index_set_genome_filter is not consulted.  opt == NULL: no flanks, errors are errors. */
enum { LM_SUBSEQ_OK = 0, LM_SUBSEQ_NO_GENOME = 1, LM_SUBSEQ_NO_SEQ = 2, LM_SUBSEQ_OUT_OF_RANGE = 3, LM_SUBSEQ_NOT_LOCAL = 4 };
#define LM_REGION_BY_NAME UINT64_MAX
typedef struct lm_region {
    uint64_t key;           /* record key, or LM_REGION_BY_NAME */
    const char *genome_id;  /* used with LM_REGION_BY_NAME */
    const char *seq_id;     /* NULL or "": see seq_idx */
    int32_t seq_idx;        /* >= 0: contig by number; < 0 with no seq_id: concatenated coordinates */
    int32_t rc;
    int64_t begin, end;     /* 1-based, inclusive */
} lm_region;
typedef struct lm_subseq_opt {
    int32_t upstream, downstream, ignore_errors, pad;
} lm_subseq_opt;
typedef struct lm_subseq_info {
    uint64_t key;           /* the record that answered (0 when none did) */
    int32_t seq_idx;        /* its contig, -1 in concatenated coordinates */
    int32_t status;         /* LM_SUBSEQ_* */
    int32_t rc, pad;
    int64_t begin, end;     /* the extracted range: start after the flank and the clamp, reported end */
    int64_t off, len;       /* into the base blob */
    const char *genome_id, *seq_id; /* borrowed from the index, valid until lm_index_close; seq_id NULL in concatenated coordinates */
} lm_subseq_info;
typedef struct lm_subseq_stats {   /* measured work of the call */
    int64_t regions, answered, bases, blob_bytes, pieces;
    double ms_plan, ms_alloc, ms_device, ms_total; /* ms_alloc: pinning the blob; ms_device: the extraction kernels alone (events around each launch) */
} lm_subseq_stats;
typedef struct lm_subseqs lm_subseqs;
void lm_subseq_opt_default(lm_subseq_opt *o);
lm_status lm_index_subseqs(lm_index *idx, const lm_region *regions, size_t n, const lm_subseq_opt *opt, lm_subseqs **out);
/* the subject region of every row: key = batch_genome, contig seq_idx, tbegin + 1 .. tend + 1, strand rc (what
 * `lexicmap utils subseq -f` reads from the TSV's sgenome, sseqid, sstart, send, sstr); rows of a gathered or merged result too */
lm_status lm_index_subseq_rows(lm_index *idx, const lm_hsp *rows, size_t n, const lm_subseq_opt *opt, lm_subseqs **out);
/* `lexicmap utils genome-seqs` (genome-seqs.go:115-137): every contig of every record of the genome, whole, forward, in record
 * and contig order.  An unknown genome id is LM_ERR_ARG. */
lm_status lm_index_genome_seqs(lm_index *idx, const char *genome_id, lm_subseqs **out);
/* returns the region count; info / bases may be NULL; valid until lm_subseqs_free */
size_t lm_subseqs_get(const lm_subseqs *s, const lm_subseq_info **info, const char **bases);
void lm_subseqs_get_stats(const lm_subseqs *s, lm_subseq_stats *stats);
void lm_subseqs_free(lm_subseqs *s);
/* The FASTA text of a result, formatted by the host threads into ONE buffer (*text, *len bytes, released with lm_free).  Per
 * region with status OK: ">%s:%d-%d:%s" with the contig id (the genome id in concatenated coordinates), begin, end and strand
 * (subseq.go:632-636); the bases in lines of line_width (line_width <= 0: one line; util.go:311-347), an empty sequence as an
 * empty line; a newline.  Regions with another status print nothing (subseq.go:233-243).  With rows (as many as regions, the
 * rows lm_index_subseq_rows was given; query_ids / query_lens / nq as in lm_format_rows) the header is the long one of
 * subseq.go:204-205, 447-450, its fields the row's TSV columns as lm_format_row prints them.  A result of
 * lm_index_genome_seqs prints just ">seqid". */
lm_status lm_format_subseqs(const lm_subseqs *s, const lm_hsp *rows, const char *const *query_ids, const uint32_t *query_lens, size_t nq,
                            int line_width, char **text, size_t *len);

typedef struct lm_stage lm_stage; /* host arrays of a stage-level call, released with lm_stage_free */

/* ---------------------------------------------------------------------------------------------------------
 * Genome-sharded indexes: every rank opens the index with its shard_rank / shard_count, searches the SAME
 * query batch, and the host gathers the per-rank rows (one all-gatherv of lm_hsp records).  lm_merge_sharded then
 * produces the reference's final order per query - genomes by the similarity (bitscore * pident) of their best HSP
 * cluster, descending (lib-index-search.go:2919-2921), each genome's rows as they were - and the global `hits`
 * (search.go:463,494): what `lexicmap utils merge-search-results` does for several indexes (merge-search-results.go:142-194).
 * rows[r] / nrows[r]: the rows of rank r, grouped by query in batch order (as lm_result_rows returns them).  Host-only;
 * idx (may be NULL) re-attaches genome_id / seq_id: every shard holds the names of all genomes.  cigar/qseq/sseq/align
 * are process-local and come back NULL.  Free with lm_result_free. */
lm_status lm_merge_sharded(lm_index *idx, const lm_hsp *const *rows, const size_t *nrows, int nshards, lm_result **out);
/* The same merge with the printer's flags: flags = 0 is lm_merge_sharded.  flags = LM_ROW_ALL (-a/--all): the cigar / qseq /
 * sseq / align pointers of the input rows are live in THIS process (e.g. the rows lm_gather_rows_ex returns with LM_ROW_ALL)
 * and every string is copied into storage the result owns, following its row into the merged order; a NULL string stays NULL,
 * "" stays "".  Other bits: LM_ERR_ARG. */
lm_status lm_merge_sharded_ex(lm_index *idx, const lm_hsp *const *rows, const size_t *nrows, int nshards, int flags, lm_result **out);

/* The ONE collective of the sharded search (north_star: "per-shard hit lists merged with a single RCCL all-gatherv over
 * xGMI"), behind the C-ABI so that the Go host needs nothing else: a gatherv of lm_hsp records to the merging rank - an
 * all-gather of the counts (24 bytes per rank), then one group of point-to-point transfers into the root ((N-1) payloads
 * over the root's xGMI links; the ranks that do not merge receive nothing).  What the gathered rows are merged into:
 * lm_merge_sharded above (lib-index-search.go:2919-2921, merge-search-results.go:142-194).
 *   lm_comm_unique_id: rank 0 makes the 128-byte id (an ncclUniqueId) and hands it to the other ranks by the host's own
 *     means (the Go host: a file, a socket or its launcher's environment; bench.py: torch.distributed broadcast);
 *   lm_comm_init: every rank, once per process - one process per GPU, `device` = the GPU of this rank's index handle;
 *   lm_gather_rows: rows / n = this rank's rows (host memory, e.g. lm_result_rows).  nrows[lm_comm_size] receives every
 *     rank's count on every rank.  On `root`, *all_rows = the rows of rank 0, 1, ... back to back (pointer columns cleared:
 *     they are addresses of other processes; lm_merge_sharded re-attaches genome_id / seq_id), owned by the communicator
 *     and valid until its next call; elsewhere *all_rows = NULL.  All ranks must call it, in the same order.
 * RCCL is bound at run time (librccl.so.1; LM_RCCL_LIB overrides): a single-GPU user never loads it.
 *
 * The _ex forms take the printer's flags: flags = 0 is the plain call, LM_ROW_ALL (-a/--all) makes the four string columns
 * travel with their rows.  ALL RANKS MUST PASS THE SAME FLAGS: every rank's flags go with its row count, and on a mismatch
 * (or a bit other than LM_ROW_ALL) every rank returns LM_ERR_ARG.  With LM_ROW_ALL the root's rows carry cigar / qseq / sseq /
 * align pointers into a pinned host buffer owned by the communicator, valid until its next call (the lifetime of the rows); a
 * NULL string comes back NULL, "" comes back "".
 *   Wire form of the strings: per row four uint32 lengths (0xFFFFFFFF = NULL) and one block `cigar\0qseq\0sseq\0align\0` (a
 *   NULL string takes no byte) zero-padded to a multiple of 16 bytes; the blocks of a rank's rows back to back in row order.
 *   Each rank sends its rows, lengths and blocks as one group (16 bytes per row plus the padded strings beside the 168-byte
 *   row).  The count exchange carries {rows, string bytes, flags and status} per rank - a rank that could not stage its
 *   payload makes every rank fail - and, once the root has sized and allocated everything it receives into, a second
 *   all-gather carries the root's go / no-go: if the root cannot receive, every rank returns LM_ERR_NOMEM and none waits. */
#define LM_COMM_ID_BYTES 128
typedef struct lm_comm lm_comm;
lm_status lm_comm_unique_id(uint8_t id[LM_COMM_ID_BYTES]);
lm_status lm_comm_init(const uint8_t id[LM_COMM_ID_BYTES], int nranks, int rank, int device, lm_comm **out);
void lm_comm_free(lm_comm *comm);
int lm_comm_rank(const lm_comm *comm);
int lm_comm_size(const lm_comm *comm);
const char *lm_comm_last_error(const lm_comm *comm); /* comm == NULL: the last failed lm_comm_unique_id / lm_comm_init of this thread */
lm_status lm_gather_rows(lm_comm *comm, const lm_hsp *rows, size_t n, int root, const lm_hsp **all_rows, size_t *nrows);
/* lm_gather_rows with flags (above).  With LM_ROW_ALL: rows' string pointers must be live in this process; on the root the
 * gathered rows carry theirs (genome_id / seq_id still NULL), ready for lm_merge_sharded_ex(..., LM_ROW_ALL, ...). */
lm_status lm_gather_rows_ex(lm_comm *comm, const lm_hsp *rows, size_t n, int root, int flags, const lm_hsp **all_rows, size_t *nrows);
/* lm_gather_rows + lm_merge_sharded in one call, the merge on the DEVICE: the other ranks' rows are received into device memory
 * in rank order, the root's own are uploaded beside them, the final order (the reference's, as lm_merge_sharded makes it) and the
 * global `hits` are computed there and downloaded once.  On `root`: *merged = `*total` rows in output order with genome_id /
 * seq_id re-attached from idx (the root's handle; NULL: left NULL), owned by the communicator and valid until its next call;
 * elsewhere *merged = NULL and *total = 0.  All ranks must call it, in the same order. */
lm_status lm_gather_merge_rows(lm_comm *comm, lm_index *idx, const lm_hsp *rows, size_t n, int root, const lm_hsp **merged,
                               size_t *total);
/* lm_gather_merge_rows with flags (above).  With LM_ROW_ALL the lengths and blocks of all ranks are received into device memory
 * in rank order beside the rows (borrowed from idx's scratch like the rows, else owned by the communicator), reordered there
 * into the output order by the device merge, and downloaded once with the rows: *merged carries the string pointers. */
lm_status lm_gather_merge_rows_ex(lm_comm *comm, lm_index *idx, const lm_hsp *rows, size_t n, int root, int flags, const lm_hsp **merged,
                                  size_t *total);
/* The merging rank's part of lm_gather_merge_rows by itself: d_rows = the rows of shard 0, 1, ... back to back in DEVICE memory
 * (nrows[r] each), merged on the device on the communicator's stream (a single-rank communicator will do), downloaded once,
 * names re-attached.  *merged / *total as above.  (How bench.py times the merge of N shards' rows on one GPU.) */
lm_status lm_merge_sharded_device(lm_comm *comm, lm_index *idx, const void *d_rows, const size_t *nrows, int nshards,
                                  const lm_hsp **merged, size_t *total);
/* lm_merge_sharded_device with flags.  flags = 0: d_strings and string_bytes are ignored (the plain call).  flags = LM_ROW_ALL:
 * d_strings = the string columns of the rows of d_rows in DEVICE memory, in the wire form above, all shards back to back:
 *     uint32 lens[total][4]        (total = the sum of nrows; shard order, then row order - as d_rows)
 *     char   blocks[string_bytes]  at d_strings + 16 * total, 16-byte aligned (d_strings itself 16-byte aligned)
 * string_bytes must be the sum of the rows' block sizes (LM_ERR_ARG otherwise, before anything is copied).  *merged carries
 * the string pointers (into the communicator's pinned buffer, valid until its next call). */
lm_status lm_merge_sharded_device_ex(lm_comm *comm, lm_index *idx, const void *d_rows, const size_t *nrows, const void *d_strings,
                                     uint64_t string_bytes, int nshards, int flags, const lm_hsp **merged, size_t *total);

/* -n/--top-n-genomes with a sharded index: the cut of lib-index-search.go:1781-1805 is over the genomes of ALL shards.
 *   1. every rank: lm_search_scores -> its candidates, per query at most top_n (query, genome, Chainer score)
 *   2. host: gather the candidates of all ranks; lm_topn_merge -> the global top-N per query (score descending, ties by
 *      genome key ascending: the total order this build uses where the reference's unstable sort leaves ties open)
 *   3. every rank: lm_search_resident_keep with that list instead of its local cut.
 * Unsharded indexes do the cut inside lm_search_resident. lm_topn_merge output arrays are released with lm_free. */
lm_status lm_search_scores(lm_index *idx, lm_qbatch *qb, lm_stage **out, size_t *n, const uint32_t **query,
                           const uint64_t **batch_genome, const float **score);
lm_status lm_topn_merge(int nshards, const uint32_t *const *query, const uint64_t *const *batch_genome,
                        const float *const *score, const size_t *n, int top_n, uint32_t **out_query,
                        uint64_t **out_batch_genome, size_t *out_n);
lm_status lm_search_resident_keep(lm_index *idx, lm_qbatch *qb, const uint32_t *keep_query, const uint64_t *keep_batch_genome,
                                  size_t nkeep, lm_result **out);
void lm_free(void *p);

/* Genome whitelist: the `genomeIds` argument of (*Index).Search (lib-index-search.go:1191,1396,1425-1489) - seeds of other
 * genomes are ignored when anchors are assembled.  The reference derives the same kind of per-genome keep flag from
 * taxids (-t/--taxids, LCA tests against taxdump: host-side, cached per genome): the host evaluates those and passes the
 * resulting genome keys here.  keys = batch<<17|index (genomes.map.bin); n = 0 clears the filter.  Applies to the calls
 * that follow on this handle. */
lm_status lm_index_set_genome_filter(lm_index *idx, const uint64_t *batch_genome_keys, size_t n);

/* ---------------------------------------------------------------------------------------------------------
 * Stage-level entry points (inner seams) used by the parity tests. All outputs are host arrays owned
 * by the returned lm_stage object. */
void lm_stage_free(lm_stage *s);

/* lexichash MaskKnownDistinctPrefixes + low-complexity zeroing (lib-index-search.go:1212-1238):
 * kmers[nq*M]; loc_off[nq*M+1] CSR into locs[] (pos<<1|strand ascending). */
lm_status lm_mask_batch(lm_index *idx, const lm_query *queries, size_t nq, lm_stage **out, const uint64_t **kmers,
                        const int64_t **loc_off, const int32_t **locs);

/* reverse re-bucketing + seed lookup + anchor assembly (lib-index-search.go:1268-1569) and, per (query,genome),
 * ClearSubstrPairs + Chainer.Chain (:1702-1775).
 * pairs: npairs records sorted by (query, batch_genome); raw anchors and cleared anchors as CSR. */
typedef struct lm_anchor {
    int32_t qbegin, tbegin;
    uint8_t len, trc, qrc, pad;
} lm_anchor;
typedef struct lm_pair {
    uint32_t query;
    uint64_t batch_genome;
    int64_t raw_off, raw_n;         /* into raw anchors (sorted in the ClearSubstrPairs order) */
    int64_t clr_off, clr_n;         /* into cleared anchors */
    float score;                    /* Chainer.Chain best score */
    int64_t chain_off, chain_n;     /* chains of this pair: chain_ptr[chain_off .. chain_off+chain_n] */
} lm_pair;
lm_status lm_seed_chain_batch(lm_index *idx, const lm_query *queries, size_t nq, lm_stage **out, size_t *npairs,
                              const lm_pair **pairs, const lm_anchor **raw, const lm_anchor **cleared,
                              const int64_t **chain_ptr, const int32_t **chain_idx);

/* SeqComparator.Index + Compare (lib-seq_compare.go:115-159,335-522) for explicit (query, target window) problems:
 * problem i compares queries[qidx[i]] over [qbegin[i], qend[i]] with targets[i]. Results CSR by problem. */
typedef struct lm_chain2 {
    int32_t qbegin, qend, tbegin, tend;
    int32_t nanchors, matched_bases, aligned_bases_q, aligned_bases_t;
    double pident;
} lm_chain2;
lm_status lm_pseudoalign_batch(lm_index *idx, const lm_query *queries, size_t nq, const lm_query *targets,
                               const uint32_t *qidx, const uint32_t *qbegin, const uint32_t *qend, size_t nproblems,
                               lm_stage **out, const int64_t **res_off, const lm_chain2 **res);
/* The same, and the pseudo-alignment anchors the chains were made from: anchors[anchor_off[i] .. anchor_off[i+1]) are the
 * anchors emitted for problem i (window coordinates), in the order of the sorted device list (the ClearSubstrPairs order:
 * QBegin ascending, QEnd descending, TBegin ascending, strand flags). */
lm_status lm_pseudoalign_batch_ex(lm_index *idx, const lm_query *queries, size_t nq, const lm_query *targets,
                                  const uint32_t *qidx, const uint32_t *qbegin, const uint32_t *qend, size_t nproblems,
                                  lm_stage **out, const int64_t **res_off, const lm_chain2 **res,
                                  const int64_t **anchor_off, const lm_anchor **anchors);
/* The same for windows of the RESIDENT genomes: problem i compares queries[query] over [qbegin, qend] with the wlen bases
 * from base tbegin of local genome `local_genome` (concatenated-genome coordinates, as lm_index_fetch), turned into their
 * reverse complement when rc != 0.  The windows are read from the 2-bit genomes by the kernels a search runs (a search
 * never takes the ASCII path of lm_pseudoalign_batch), on a handle with host-resident genomes through its staging buffer.
 * LM_ERR_ARG with a text: a query or genome that does not exist here, tbegin < 0, wlen < 0, a window past the genome's last
 * base, qend past the query.  All regions are one chunk: one that needs more anchors than the scratch budget allows is an
 * error (LM_ERR_HIP), it is not split. */
typedef struct lm_pa_region {
    uint32_t query, qbegin, qend;
    int32_t rc;
    int64_t local_genome;
    int32_t tbegin, wlen;
} lm_pa_region;
lm_status lm_pseudoalign_regions(lm_index *idx, const lm_query *queries, size_t nq, const lm_pa_region *regions,
                                 size_t nregions, lm_stage **out, const int64_t **res_off, const lm_chain2 **res,
                                 const int64_t **anchor_off, const lm_anchor **anchors);

/* wfa.Aligner.Align(q,t) with DefaultPenalties, global, AdaptiveReduction(DefaultAdaptiveOption)
 * (lib-index-search.go:1910-1911,2261,2528). ops CSR: op<<32|n in forward order. */
typedef struct lm_wfa {
    int32_t status; /* 0 ok, 2 no match op */
    int32_t score;  /* WFA penalty score */
    int32_t qbegin, qend, tbegin, tend;
    uint32_t align_len, matches, gaps, gap_regions;
    int64_t ops_off;
    int32_t nops;
} lm_wfa;
lm_status lm_wfa_batch(lm_index *idx, const lm_query *q, const lm_query *t, size_t n, lm_stage **out,
                       const lm_wfa **res, const uint64_t **ops);

/* ---------------------------------------------------------------------------------------------------------
 * Measurement support: per-kernel HIP-event timing on the library's own stream. */
typedef struct lm_kernel_time {
    const char *name;
    int64_t launches;
    double total_ms;
    int64_t bytes;   /* algorithmic bytes accounted by the host for these launches */
} lm_kernel_time;
void lm_profile_enable(lm_index *idx, int on);
void lm_profile_reset(lm_index *idx);
/* exclusive != 0: the searches that follow run their kernels one after the other (no overlapped streams), so that the
 * per-kernel HIP-event times are exclusive times; results are unchanged. Measurement only. */
void lm_profile_exclusive(lm_index *idx, int exclusive);
size_t lm_profile_get(lm_index *idx, const lm_kernel_time **out);
/* Measurement only: waits for the device, launches the empty kernel lm::k_profile_mark(id) and waits again - a boundary a
 * rocprofv3 trace or counter pass can be cut at (tools/summarize_rocprof.py keeps the dispatches between the first two marks). */
void lm_profile_mark(lm_index *idx, int id);
/* Measurement only: re-reads the LM_* experiment switches (which a handle reads once, when it is opened or built) from the
 * environment, so that one resident index can be timed under several settings (bench.py --ab).  Results are unchanged by any
 * switch; the alignment scratch of the handle is dropped so that it is re-cut under the new settings. */
void lm_tuning_reload(lm_index *idx);

#ifdef __cplusplus
}
#endif
#endif
