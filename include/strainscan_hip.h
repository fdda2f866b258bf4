/*
 * strainscan_hip.h -- C ABI of the MI355X (gfx950) identification hot path of StrainScan.
 *
 * This is the drop-in boundary: plain C, caller-owned buffers, integer status codes (0 = ok,
 * negative = error, see ss_strerror).  Python reaches it through ctypes
 * (strainscan_amd/_lib.py); nothing in the signatures depends on PyTorch.  Each entry point
 * names the reference interface (file:line under liaoherui/StrainScan) it replaces.
 *
 * Conventions
 *   - "dev" pointers are HIP device pointers on the current device; "stream" is a hipStream_t
 *     passed as void* (NULL = the default stream).  Functions whose name ends in _dev only
 *     enqueue work on that stream; everything else is synchronous on return.
 *   - k-mer keys are 2 bits per base, FIRST base in the LEAST significant bits, with the code
 *     (ascii >> 1) & 3, i.e. A=0 C=1 T=2 G=3 (case-insensitive); k <= 31.
 *   - a "flat base block" is the device input format of the scan: the sequence bytes of the
 *     reads, one '\n' after every record.  Any byte outside ACGTacgt ends a k-mer window, so
 *     k-mers never span records and N / IUPAC codes behave as in `jellyfish count`.
 */
#ifndef STRAINSCAN_HIP_H
#define STRAINSCAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_OK 0
#define SS_EINVAL (-22)   /* bad argument */
#define SS_ENOMEM (-12)   /* host or device allocation failed */
#define SS_EIO (-5)       /* file could not be read */
#define SS_EHIP (-1000)   /* a HIP runtime call failed; ss_last_error() has the text */
#define SS_ENODEV (-19)   /* no usable GPU */
#define SS_EKEY (-2)      /* the reference would raise KeyError here */
#define SS_ERANGE (-34)   /* value out of the supported range (k > 31, p > 16, ...) */
#define SS_EAGAIN (-11)   /* strict .gz policy (ss_gz_set_policy(1)): the device path declined an input; agree with the other
                             ranks, then load again under policy 2 */

#define SS_ROW_VALID 1u   /* row flag: ACGT-only k-mer of length k */
#define SS_ROW_LOWER 2u   /* row flag: text contains lower-case letters */
#define SS_NO_SLOT 0xFFFFFFFFu

int ss_version(void);
const char *ss_strerror(int code);
const char *ss_last_error(void);         /* thread-local text of the last SS_EHIP */
int ss_device_count(int *n);             /* does not initialise the GPU runtime beyond counting */
int ss_set_device(int dev);
int ss_device_sync(void);
int ss_stream_sync(void *stream);

/* device memory helpers for callers that do not bring their own allocator */
int ss_dev_alloc(void **dptr, uint64_t bytes);
int ss_dev_free(void *dptr);
/* Stream-ordered twins on the CALLING THREAD's stream (hipStreamPerThread), from the device's memory pool: what layer 2 uses
 * for its per-call vectors, so that clusters solved on several host threads do not meet in hipFree's device-wide
 * synchronisation.  A buffer must be freed by the thread that used it last (strainscan_amd/l2.py DevBuf falls back to
 * ss_dev_free otherwise). */
int ss_dev_alloc_async(void **dptr, uint64_t bytes);
int ss_dev_free_async(void *dptr);
int ss_memcpy_h2d(void *dst_dev, const void *src, uint64_t bytes, void *stream);
int ss_memcpy_d2h(void *dst, const void *src_dev, uint64_t bytes, void *stream);
int ss_memset_dev(void *dst_dev, int byte, uint64_t bytes, void *stream);

/* --------------------------------------------------------------------------------------------
 * seqpy.revcomp  (library/seqpy.c:24-36): reverse + IUPAC complement, case preserved.
 * ss_revcomp is the host form (what the CPython extension did); ss_revcomp_dev runs the same
 * table on the GPU for n_seq equal-length sequences stored back to back.
 * ------------------------------------------------------------------------------------------ */
int ss_revcomp(const char *in, char *out, uint64_t n);

/* CPUs this process may use: hardware threads capped by the cgroup CPU quota (SS_HOST_CPUS overrides).  The host-side
 * thread pools (parsers, inflater, index build) size themselves with it. */
int ss_host_cpus(void);

/* Whole-file gunzip as ss_scan_files / ss_reads_load do it for .gz inputs (the reference pipes `zcat`,
 * identify.py:81-84).  mode 0: one gzip member is inflated by `threads` threads (0 = all, up to 32) when it is
 * large enough -- entry points found inside the deflate stream, chunks decoded against an unknown 32 KB window
 * and resolved afterwards, result verified against the member's CRC-32 and length -- else by libdeflate;
 * 1: the threaded inflater or nothing; 2: libdeflate only.  SS_ERANGE = not inflated here (not gzip, too small,
 * several members, over the memory budget, verification failed): stream it with zlib.  *text is released with
 * ss_gz_free.  Host only. */
int ss_gz_inflate(const char *path, int threads, int mode, char **text, uint64_t *len);
void ss_gz_free(char *text);
/* The same text written to out_path (the threaded inflater writes through a shared mapping of the file): the ranks
 * of one node inflate a .gz sample ONCE into /dev/shm and each parses its share of the plain text. */
int ss_gz_inflate_to_file(const char *path, const char *out_path, int threads, uint64_t *len);
/* The same on the GPU (ss_ginflate.hip, its kernels in ss_ginflate_dev.h: the two-pass scheme with one wave per chunk of the deflate data, the
 * text verified against CRC-32 and ISIZE of the trailer); *text is a host buffer released with ss_gz_free.  SS_ERANGE:
 * not handled on the device (a damaged file, data that expands beyond the symbol budget, ...): use ss_gz_inflate. */
int ss_gz_inflate_gpu(const char *path, char **text, uint64_t *len);
/* Members the device inflater has produced / has declined in this process.  Unless SS_GZ_GPU=0, the .gz inputs of
 * ss_scan_files and ss_reads_load (one rank, files of 1 MB and more) go through it first and strict four-line FASTQ is
 * reduced to its sequence lines on the device too (ss_fastq_dev.hip); what it declines goes to the host inflaters. */
int ss_gz_gpu_counters(uint64_t *handled, uint64_t *declined);
/* The device inflater keeps its scratch (symbol streams, window maps, the text buffer: ~6-12 GB, at most two sets; its
 * pinned upload buffers) for the next call, the binning of resident reads its 0.2 GB -- large allocations are slow to come
 * by on this platform; this hands all of it back, and the large device blocks kept by ss_dev_big_blocks' stash
 * (ss_gz_scratch.hip). */
int ss_gz_gpu_release(void);
/* Device blocks of 256 MB and more that a load is done with -- the text of a large .gz, the file-order slab that binning has
 * replaced, the slabs of a destroyed read set -- are kept (at most three, 24 GB) and handed to the next large request of this
 * process (slabs, binned slabs, .gz texts) instead of going back to the driver, which hands fresh device memory out at
 * ~25 GB/s (ss_host.hip ss::big_take).  out[0] = blocks kept now, out[1] = their bytes, out[2] = requests served from kept blocks. */
int ss_dev_big_blocks(uint64_t out[3]);
/* A block is tagged with the device it lives on and is only ever served to a request made under that device (ss_set_device).
 * A caller that shares the GPU with other allocators (torch, another library) and wants the kept blocks back in the driver's
 * hands calls this: every kept block is hipFree'd.  (ss_gz_gpu_release does the same and more.) */
int ss_dev_big_release(void);
/* The pinned upload buffers of n_files (<= 2) concurrent .gz inputs, made ahead of time (~40 ms a set; a command-line process
 * calls this on its warm-up thread): a file of 32 MB or more then travels through them (8 ms instead of 12-30 per 66 MB);
 * without them only files of 256 MB or more make their own (ss_gz_scratch.hip). */
int ss_gz_warm_up(int n_files);
/* Who inflates the .gz inputs of the next ss_reads_load / ss_scan_files* calls of this process: 0 (default) the device, and
 * the host inflaters for whatever it declines; 1 the device or NOBODY -- a declined input makes the call return SS_EAGAIN
 * with nothing loaded; 2 the host inflaters.  The two paths give a rank different shares of the reads (blocks of 4096
 * records / parse chunks), and the device path can decline for reasons of its own (free memory, a HIP error), so the
 * ranks of a sharded run must all take the same path for a file: they load under policy 1, all-reduce the outcome and,
 * if any of them was declined, all load again under policy 2 (strainscan_amd/dist.py load_agreed). */
int ss_gz_set_policy(int mode);
/* Several ranks SHARE the inflation of a gzip member (ss_gz_range.hip: the chain; ss_ginflate.hip: the slices; the reference pipes one `zcat` per file,
 * identify.py:81-84).  The deflate data is cut into slices, slice s belongs to rank s mod world: a rank finds the block
 * starts of its slices, inflates them to symbols (the expensive part, all ranks at once) and receives what lies in front
 * of each slice -- 32 KB of text, the count of newlines so far, the bytes of the record that straddles the cut, CRC-32 and
 * length so far -- from the owner of the slice before, through `chain`: direction 0 = fill msg with what the owner of
 * slice - 1 sent, 1 = send msg to the owner of slice + 1 (blocking; return 0, anything else breaks the chain off).  The
 * rank keeps ALL records that begin in its slices (no further sharding of these files).  One member, several members
 * joined with cat, or bgzip (a slice = the members that begin in its byte range).  Active while world > 1 and chain
 * != NULL, and only under policy 1: a rank that cannot take part (a wrong entry at a slice's edge, no room, text that
 * is not four-line FASTQ, ...) still serves the chain, passes the bad news on and returns SS_EAGAIN; the ranks then settle for the
 * whole-file path (range off) or the host inflaters.  slice_bytes = 0: file size / (2 world), 4 MB .. 128 MB. */
typedef int (*ss_gz_chain_fn)(void *msg, uint64_t bytes, int slice, int direction, void *user);
int ss_gz_set_range(int rank, int world, uint64_t slice_bytes, ss_gz_chain_fn chain, void *user);
/* files this process has inflated its share of in range mode, and the slices that came to */
int ss_gz_range_counters(uint64_t *files, uint64_t *pieces);
/* Test hooks (ss_host.hip), switched by this call only (nothing in the environment does): which = 1: plant a wrong block entry in search
 * chunk `value` of every .gz inflated on the device (0 = off); 2: this process declines .gz inputs on the device (in range mode
 * it still serves the chain); 3: this rank leaves range mode WITHOUT serving the chain -- what a crashed peer looks like;
 * 4: which scan kernel of the page index a table goes through -- value 1: tables of k = 31 through the one-lane-per-position
 * kernel, 2: tables of every k through it, 3: tables of every k through the run-queue kernel (k at run time), 0: the product's choice
 * -- so that a test can hold the kernels to each other on one index; 5: the layout of binned slabs of records of one length --
 * value 1: they stay ASCII, 0: the product's choice (2-bit codes + invalid flags, 3 bytes per 8 positions, where every record
 * byte is A C G T or N; see ss_reads_packed_slabs) -- so that a test can hold the two layouts to each other on one read set;
 * 6: how binned slabs of records of one length are made -- value 1: the count pass + atomic placement (records in a bin in
 * no fixed order), 0: the product's choice (keys, a stable radix sort, a gather: records in a bin in file order) -- so that a
 * test or an A/B run can hold the two to each other in one process; 7: value 1: the device walk of a BAM stream declines, as
 * after its re-walk rounds run out -- ss_reads_load decodes the BAM on the host, ss_bam_select / ss_bam_extract take the record
 * starts from the host's walk. */
int ss_test_hook(int which, long long value);

/* The test sets of ShuffleSplit(n_splits, test_size, random_state=seed).split(range(n)) as scikit-learn 0.23
 * draws them for ElasticNetCV (identify_strains_L2_Enet_Pscan_new_sp.py:436-442: cv=ShuffleSplit(20, test_size=.5,
 * random_state=0)): bits[i] bit f = row i is in the test set of split f (the first n_test entries of the f-th
 * numpy.random.RandomState(seed).permutation(n)).  Host only; n < 2^32, n_splits <= 31. */
int ss_shuffle_split_bits(uint64_t n, int n_splits, uint64_t n_test, uint32_t seed, uint32_t *bits);
int ss_revcomp_dev(const char *in_dev, char *out_dev, uint64_t seq_len, uint64_t n_seq, void *stream);

/* --------------------------------------------------------------------------------------------
 * k-mer FASTA rows  (the `--if <db>/kmer.fa` / `all_kmer.fasta` argument of
 * library/identify.py:82-86 and library/Vote_Strain_L2_Lasso_new_sp.py:359-371, and the
 * kmer_index_dict loop of identify.py:90-95).
 * Row i = i-th record (line 2i+1).  A row whose text is an ACGT-only k-mer (either case) gets
 * SS_ROW_VALID and its 2-bit key; other rows get flags 0.
 * ------------------------------------------------------------------------------------------ */
int ss_kmerfa_count_rows(const char *path, uint64_t *n_rows);
/* <Tree_database>/kmers/<id> (one line of 0-based row numbers of kmer.fa each, Build_tree.py:686-698; read by match_node,
 * identify.py:116-118) for all listed ids, on the host's threads.  rows == NULL: counts[i] = row numbers of file i; else they are
 * written to rows + offsets[i] (counts from the first call are checked).  A token that is not a decimal number below n_rows:
 * SS_EINVAL, *bad = index of the first such file.  Host only. */
int ss_node_lists_parse(const char *kmers_dir, const long long *ids, uint32_t n_ids, uint64_t n_rows, uint64_t *counts,
                        const uint64_t *offsets, uint32_t *rows, uint32_t *bad);
int ss_kmerfa_encode(const char *path, int k, uint64_t n_rows, uint64_t *keys, uint8_t *flags, int threads);
/* same on an in-memory text */
int ss_kmerfa_encode_mem(const char *text, uint64_t len, int k, uint64_t n_rows, uint64_t *keys, uint8_t *flags);
/* one ASCII k-mer -> key; returns SS_EINVAL if it is not ACGT-only */
int ss_encode_kmer(const char *kmer, int k, uint64_t *key);

/* --------------------------------------------------------------------------------------------
 * Device k-mer database = what `jellyfish count --if` builds from the FASTA
 * (identify.py:82-86): an open-address table of the distinct valid row k-mers.
 *   upper_keys = 1: identify.py semantics (dict keyed by .upper(), identify.py:94)
 *   upper_keys = 0: identify_low_mem.py:81 / identify_low_depth.py:64 (raw keys): a lower-case
 *                   row never owns a k-mer; ss_db_build returns SS_EKEY when a k-mer is left
 *                   without an owning row (the reference raises KeyError at :88).
 *   upper_keys = 2: raw keys, lenient -- Vote_Strain_L2_Lasso_new_sp.py:312-322 looks each
 *                   all_kid.pkl key up in the dump and takes 0 when it is absent, so a lower-case
 *                   row simply never gets a count.
 * Duplicate k-mers: the LAST row owns the count (dict overwrite); earlier rows are not valid.
 * ------------------------------------------------------------------------------------------ */
typedef struct ss_db ss_db;
int ss_db_build(const uint64_t *keys, const uint8_t *flags, uint64_t n_rows, int k, int upper_keys,
                ss_db **out);
int ss_db_destroy(ss_db *db);
int ss_db_info(const ss_db *db, uint64_t *n_rows, uint64_t *n_distinct, uint64_t *capacity, int *k);
/* The built index as a file (device arrays dumped verbatim): a database is indexed once, later
 * runs import the image.  Only the k = 31 minimizer layout is exported (SS_ERANGE otherwise);
 * ss_db_import returns SS_EINVAL / SS_EIO for anything that is not a complete image. */
int ss_db_export(const ss_db *db, const char *path);
int ss_db_import(const char *path, ss_db **out);
/* row_valid[i] = 1 iff row i is a key of the reference's match_results (identify.py:96-101) */
int ss_db_row_valid(const ss_db *db, uint8_t *row_valid);
const uint8_t *ss_db_row_valid_dev(const ss_db *db);
uint64_t ss_db_device_bytes(const ss_db *db);
/* Shape of the built index, for benchmarks and logs (no reference counterpart: jellyfish prints nothing):
 * out[0] layout (0 flat table, 1 minimizer pages), [1] counters, [2] minimizers, [3] 64-byte pages,
 * [4] log2 of the filter size in bits (0 = none), [5] distinct k-mers, [6] bucket-array slots, [7] k-mers inline in pages. */
int ss_db_index_info(const ss_db *db, uint64_t out[8]);
/* A hint, not a semantic switch (counts are the same either way): most k-mers of the reads ARE in this table -- a layer-2
 * cluster table, all_kmer.fasta of a cluster the sample was found to contain (Vote_Strain_L2_Lasso_new_sp.py:354-372; the
 * reference runs the same jellyfish command for it as for the tree).  Scans of such a table skip the minimizer filter and,
 * for a resident read set in locality order, add the hits of neighbouring reads up in LDS before they go to the counters
 * (ss_mini.hip: a global atomic costs the same whatever it carries, 27 G line requests/s on MI355X). */
int ss_db_expect_hits(ss_db *db, int expect);
/* What the scan of a binned resident read set (ss_reads) learnt about a table nobody has flagged: the set's first 8192
 * tiles run through the plain kernel and report their found runs; at 8 per tile and above the rest of the set goes through
 * the combining kernel (hits added up in LDS).  out[0] = serial of the read set last probed (0: none yet), [1] = 1 when the
 * combining kernel was chosen, [2] = found runs per tile, times 1000.  One probe per (read set, table); no reference
 * counterpart (jellyfish has one counting loop). */
int ss_db_probe_info(const ss_db *db, uint64_t out[3]);

/* --------------------------------------------------------------------------------------------
 * The scan  (the `jellyfish count` + `dump -c` pair of identify.py:82-87,
 * identify_low_mem.py:73-75, identify_low_depth.py:53-59, Vote_...:359-372).
 * Counts accumulate in the db handle until ss_scan_reset.
 *   ss_scan_flat_dev : flat base block already in HBM (n bytes), enqueued on `stream`
 *   ss_scan_flat_host: flat base block in host memory; staged through pinned buffers, overlapping
 *                      copies with kernels; synchronous
 *   ss_scan_files    : FASTA/FASTQ files (plain or .gz), parsed on the host the way jellyfish
 *                      reads them (multi-line records, '+'/'@' quality lines), then scanned
 *                      (on streams of the parser's own: the call first waits for what is pending on
 *                      the default stream -- an ss_scan_reset(db, NULL) just before it)
 *   ss_scan_reset    : zeroes the counters, asynchronously on `stream`
 * ------------------------------------------------------------------------------------------ */
int ss_scan_reset(ss_db *db, void *stream);
int ss_scan_flat_dev(ss_db *db, const void *bases_dev, uint64_t n, void *stream);
int ss_scan_flat_host(ss_db *db, const char *bases, uint64_t n);
int ss_scan_files(ss_db *db, const char *const *paths, int n_paths, uint64_t *n_records, uint64_t *n_bases);
/* The same for one rank of a sharded scan (reads shard across GPUs): only the chunks c of the input with
 * c % shard_world == shard_rank are parsed, copied and scanned (the sequential reader, where a file needs it, walks
 * everything and keeps every shard_world-th block).  n_records / n_bases: this rank's share for chunk-parsed files. */
int ss_scan_files_shard(ss_db *db, const char *const *paths, int n_paths, int shard_rank, int shard_world,
                        uint64_t *n_records, uint64_t *n_bases);
/* counts per ROW (match_results as an array; 0 for rows that are not valid) */
int ss_counts_rows_dev(const ss_db *db, uint32_t *counts_rows_dev, void *stream);
int ss_counts_rows(const ss_db *db, uint32_t *counts_rows);
/* replace the accumulated counts by the given per-row counts (multi-GPU: every rank scans its
 * read shard, the uint32[n_rows] vectors are sum-all-reduced over RCCL, and each rank loads the
 * global vector back so that all later reductions see whole-sample counts) */
int ss_counts_load_rows_dev(ss_db *db, const uint32_t *counts_rows_dev, void *stream);
uint64_t ss_scan_kernel_launches(const ss_db *db);   /* scan kernels enqueued so far (diagnostics) */

/* --------------------------------------------------------------------------------------------
 * Resident read sets.  The reference re-reads the FASTQ for the tree scan, for every identified
 * multi-strain cluster and twice more with -b (identify.py:409; Vote_Strain_L2_Lasso_new_sp.py:
 * 354-372; identify_low_depth.py:119,124).  Counting does not depend on the order of the records, so the resident
 * records CAN be kept in locality order -- sorted by the minimizer of their first k-mer, reads that start within the same
 * 17 bases of a genome become neighbours and share their page lookups: scans 20-35 % faster at high coverage, 3.5 ms
 * per 20 M reads once (ss_reorder.hip; the default since round 3, SS_READS_ORDER=file keeps the file order: it pays from
 * the second scan of a sample on, a sample that is scanned once loses ~1.4 ms per 20 M reads).  ss_reads_load parses the files ONCE (worker threads
 * for plain files) and keeps the flat base blocks in HBM; ss_scan_reads scans them against any
 * database image.  shard_rank / shard_world: keep every shard_world-th block (multi-GPU).
 * ------------------------------------------------------------------------------------------ */
typedef struct ss_reads ss_reads;
int ss_reads_load(const char *const *paths, int n_paths, int shard_rank, int shard_world, ss_reads **out);
/* The one-time costs of the first ss_reads_load of a process (pinned parse buffers, streams: ~0.1 s), paid ahead of time --
 * a command-line process calls it on a worker thread while the interpreter starts up. */
int ss_ingest_warm_up(void);
/* FASTQ parse threads a load of this process uses: min(20, CPUs this process may use / LOCAL_WORLD_SIZE) -- the cgroup quota
 * counts, and the ranks of one node (one process per GPU under torchrun) share it; SS_INGEST_THREADS overrides. */
int ss_ingest_threads(int *n);
/* A resident read set from a flat base block that is already on the device (copied; order != 0: its records are put
 * in locality order, see below).  Its records are not counted here: the first ss_reads_info that asks for n_records counts
 * them on the device (one pass over an ASCII slab; a packed slab knows). */
int ss_reads_from_flat_dev(const void *flat_dev, uint64_t n, int order, ss_reads **out);
/* The records of a set that is in file order (ss_reads_from_flat_dev with order = 0, what ss_reads_select and ss_reads_resample
 * return) put in locality order in place, whatever SS_READS_ORDER says: every slab that is not binned yet is replaced by its binned
 * (where its records allow it: packed) copy; slabs below 64 bytes stay.  The records and every count are unchanged.  Waits for the
 * device first (a scan in flight reads the slabs that are replaced).  SS_EINVAL: NULL. */
int ss_reads_order(ss_reads *r);
/* Where the last binning of a read set spent its time, in ms.  Records of one length (the sorted path): out[0] key pass + radix
 * sort (device time), out[1] the driver's allocation of the new slab (0.3 ms, or 60-90 ms for 3 GB on a box whose driver clears
 * the memory first), out[2] gather + tail (and the ASCII gather again where a byte is not A C G T N).  The general passes and
 * ss_test_hook 6: out[0] count pass + prefix over the bins, out[1] the allocation, out[2] place pass. */
int ss_reads_order_timing(double out_ms[3]);
/* Slabs this process has binned so far: out[0] through the passes for records of ONE length (every record of the slab as long
 * as its first: a sequencer's 150-base reads; the key and gather passes check every record and a single exception sends the slab through
 * the general passes), out[1] through the general passes (ragged records).  SS_ORDER_FIXED=0 switches the former off. */
int ss_reads_order_counters(uint64_t out[2]);
/* The resident flat blocks copied back to the host, slab after slab (host = NULL: only *len); for tests and debugging. */
int ss_reads_read_back(const ss_reads *r, char *host, uint64_t cap, uint64_t *len);
/* How many of the set's slabs are PACKED: binned records of one length whose every byte is A C G T or N, held as 2-bit codes
 * and invalid flags (57 bytes for a 150-base read instead of 152); the scans read them as they are, ss_reads_read_back
 * returns the bytes their ASCII form would hold.  Slabs with any other byte (lower case, IUPAC codes, '\r') stay ASCII. */
int ss_reads_packed_slabs(const ss_reads *r, uint64_t *n_packed);
/* Lifetime: ss_scan_reads / ss_scan_reads_multi are asynchronous on the caller's stream and read the set's slabs.  Destroying
 * a set WAITS for the device (hipDeviceSynchronize) before its slabs are given up -- the large ones are kept for the next load
 * of this process (ss_dev_big_blocks), the rest go back to the driver -- so a scan still in flight on any stream finishes on
 * intact bases, as it did when the slabs were hipFree'd.  The counters of the scan belong to the ss_db, not to the read set. */
int ss_reads_destroy(ss_reads *r);
int ss_reads_info(const ss_reads *r, uint64_t *n_records, uint64_t *n_bases, uint64_t *n_blocks,
                  uint64_t *device_bytes);
/* Asynchronous on `stream`, with one exception: the FIRST scan of a (read set, table) pair whose table was not announced
 * with ss_db_expect_hits probes the set's first tiles and waits for their answer (one stream synchronisation, ~40 us of
 * kernel) before it launches the rest -- that call cannot be captured into a hipGraph; every later scan of the pair can. */
int ss_scan_reads(ss_db *db, const ss_reads *r, void *stream);
/* The same reads against several tables in ONE pass (the reference's loop over the identified clusters,
 * Vote_Strain_L2_Lasso_new_sp.py:295-296, re-reads the FASTQ for each, :354-372): equal to ss_scan_reads on each table;
 * k = 31 tables share the encoding and the minimizer runs of every tile, four tables per launch. */
int ss_scan_reads_multi(ss_db *const *dbs, int n_dbs, const ss_reads *r, void *stream);
/* Launches of the several-tables kernel so far in this process, per filter kind of the tables it took (diagnostics):
 * out[0] tables behind their own Bloom filters (tree tables), out[1] tables announced with ss_db_expect_hits, out[2] neither. */
int ss_scan_multi_launches(uint64_t out[3]);
/* How many records of a resident set carry k-mers of a table (`--read_support`).  A record is a maximal run of bytes other than
 * '\n' in the set (a read; a record longer than a block counts as its pieces); a hit of a record is a k-mer start position in it at
 * which ss_scan_reads would add 1 to a counter of the table.
 * hist[b], b < n_bins-1: records of the set with exactly b hits against db; hist[n_bins-1]: records with >= n_bins-1.
 * *hits: the hits of all records.  sum(hist) = the set's non-empty records.  Reads the table's index, never its counters
 * (a scan's accumulated counts are the same before and after).  Synchronous.  Page-index tables (17 <= k <= 31) only:
 * SS_ERANGE for a flat table; SS_EINVAL for n_bins < 2, a NULL argument, a table and a set on different devices. */
int ss_reads_support(const ss_db *db, const ss_reads *r, uint32_t n_bins, uint64_t *hist, uint64_t *hits);
int ss_reads_support_calls(uint64_t *n);   /* calls so far in this process (diagnostics; tests use it to show "flag off = not run") */
/* The records of a resident set with at least min_hits hits against a table, as a NEW resident set (`--extract_reads`); a record
 * and a hit are those of ss_reads_support.  *out is destroyed by the caller like any other set.  It holds exactly the selected
 * records, in an unspecified order, as one ASCII, unbinned slab in the flat layout (each record's bytes and '\n', the block padded
 * with '\n'); nothing selected: a valid set of 0 records.  From an ASCII slab the bytes are copied as they are (lower case, IUPAC
 * codes, '\r'); from a packed slab a base is the letter ss_reads_read_back writes.  ss_reads_read_back, ss_reads_info (n_records
 * and n_bases exact), ss_scan_reads and ss_reads_support work on *out unchanged.  Synchronous.  Reads the table's index, never its
 * counters.  SS_ERANGE: a flat table (k below 17); a set with a cut record, at any k (a cut piece is not a read); more records
 * than hipcub's int item count holds.  SS_EINVAL: a NULL argument, min_hits == 0, a table and a set on different devices. */
int ss_reads_select(const ss_db *db, const ss_reads *r, uint32_t min_hits, ss_reads **out);
int ss_reads_select_calls(uint64_t *n);    /* calls so far in this process (diagnostics; "flag off = not run") */
/* The same two questions per LABEL of the table's rows (`--by_strain`: a cluster table holds the k-mers of all its strains; the
 * caller labels the rows that only one of the called strains has).  row_labels[i], i < the table's rows (host memory): 0 = the row
 * counts for nobody, j in 1..n_labels = it counts for label j.  Rows that share a slot (the same k-mer listed twice) keep their
 * common label; where they disagree the k-mer counts for nobody.  A hit of label j is a hit of ss_reads_support whose k-mer has
 * label j, so label j's results are those of ss_reads_support / ss_reads_select against a table of label j's k-mers alone.
 * ss_reads_support_labeled: hist[(j-1) * n_bins + b] and hits[j-1] as ss_reads_support defines them, kmers[j-1] = the distinct
 *   k-mers (slots) of label j.  Each label's histogram sums to the set's records.
 * ss_reads_select_labeled: ss_reads_select on the hits of `label`.
 * Both are synchronous and read the table's index, never its counters.  SS_ERANGE: as the unlabelled call states it.  SS_EINVAL:
 * as there, and n_labels outside 1..SS_LABELS_MAX, a row label above n_labels, `label` outside 1..n_labels. */
#define SS_LABELS_MAX 15
int ss_reads_support_labeled(const ss_db *db, const ss_reads *r, const uint8_t *row_labels, uint32_t n_labels, uint32_t n_bins,
                             uint64_t *hist, uint64_t *hits, uint64_t *kmers);
int ss_reads_select_labeled(const ss_db *db, const ss_reads *r, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                            uint32_t min_hits, ss_reads **out);
int ss_reads_labeled_calls(uint64_t *n);   /* calls of either so far in this process (diagnostics; "flag off = not run") */
/* A resident set resampled with replacement, as a NEW resident set (`--bootstrap`): every record of r (a record is that of
 * ss_reads_support) appears in *out w times, w in 0..13, a Poisson(1) draw.  The layout of *out is that of ss_reads_select: one
 * ASCII, unbinned slab, each copy's bytes and '\n', the block padded with '\n', letters from a packed slab as ss_reads_read_back
 * writes them, n_records and n_bases of ss_reads_info exact, the order unspecified; nothing drawn: a valid set of 0 records.
 * w depends on the record's BYTES only, so file order, binned ASCII, packed slabs and any sharding over ranks draw the same
 * weight for the same read -- and identical reads share a weight.  It is, all arithmetic mod 2^64:
 *   key = the second 64-bit half of the record's digest (keys[2i + 1] of ss_flat_record_keys) over its flat bytes; from a
 *         packed slab these are the letters of its ASCII form
 *   x = key + 0x9E3779B97F4A7C15 * (replicate + 1) + 0xD6E8FEB86659FD93 * seed
 *   x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;  x = (x ^ x >> 27) * 0x94D049BB133111EB;  x ^= x >> 31;  u = x >> 32
 *   w = the number of entries T_k <= u of T_k = floor(2^32 * e^-1 * sum_{i <= k} 1/i!), k = 0..12:
 *       1580030168 3160060337 3950075421 4213413783 4279248373 4292415291 4294609777
 *       4294923276 4294962463 4294966817 4294967252 4294967292 4294967295
 * Synchronous.  SS_EINVAL: a NULL argument.  SS_ERANGE: a set with a cut record; more records than hipcub's int item count holds. */
int ss_reads_resample(const ss_reads *r, uint64_t seed, uint32_t replicate, ss_reads **out);
int ss_reads_resample_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* The counts of several bootstrap replicates from ONE pass over the resident reads (`--bootstrap_clusters`): no replicate is
 * materialised.  counts_rows_dev[j * n_rows + i] is, bit for bit, what ss_counts_rows_dev returns for row i after these three
 * steps on a table with the same index:
 *   1. ss_scan_reset
 *   2. ss_scan_reads of the set ss_reads_resample(r, seed, first_replicate + j) returns
 *   3. the read-out itself
 * Equivalently, it is the sum over the records of r of w(record, seed, first_replicate + j) times the record's hits on the row's
 * k-mer.  A record, a hit and w are those of ss_reads_support and ss_reads_resample.  Row validity and duplicate rows follow
 * ss_counts_rows_dev (the last row owns the count).
 * Synchronous.  Reads the table's index, never its counters (a scan's accumulated counts are the same before and after).  Works
 * on any resident set (file order, binned ASCII, packed, several slabs) and on page-index tables at 17 <= k <= 31, behind a Bloom
 * filter or flagged with ss_db_expect_hits.  counts_rows_dev is device memory; every entry is written, so the caller need not
 * clear it.  The call takes n_replicates x the table's slots x 4 bytes of device scratch for its length.
 * SS_ERANGE: a flat table (k below 17); a set with a cut record.  SS_EINVAL: a NULL argument; n_replicates outside
 * 1..SS_SCAN_REPLICATES_MAX; a table and a set on different devices. */
#define SS_SCAN_REPLICATES_MAX 16
int ss_scan_reads_resampled(const ss_db *db, const ss_reads *r, uint64_t seed, uint32_t first_replicate, uint32_t n_replicates,
                            uint32_t *counts_rows_dev /* [n_replicates][n_rows] */);
int ss_scan_reads_resampled_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* Every record of a resident set assigned to a node of a tree over the table's k-mers (`--classify_reads`); a record and a hit are
 * those of ss_reads_support.  row_node[i], i < the table's rows (host memory): 0 = the row counts for nobody, v in 1..n_nodes = it
 * is a k-mer of node v.  Rows that share a slot (the same k-mer listed twice) keep their common node; where they disagree the
 * k-mer counts for nobody.  parent[v], v in 1..n_nodes (parent[0] is not read): v's parent, 0 = none; the array must describe a
 * forest (parent[v] < v is not required), which is checked on the host before anything is launched.
 *   h[v]     = the record's hits whose k-mer has node v
 *   score(v) = the sum of h[u] over the path from v's root to v, v included, for every v with h[v] > 0
 *   class    = the node with the largest score; several nodes with that score (never on one path): their lowest common ancestor,
 *              which may have no hits itself, and 0 when they stand in different trees; 0 (unclassified) when the largest score
 *              is below min_score or no hit has a node
 * direct[c], c in 0..n_nodes: records of class c; sum(direct) = the set's non-empty records.  node_hits[v]: the sum of h[v] over
 * all records, node_hits[0] the hits of k-mers without a node.  kmers[v]: the distinct k-mers (slots) of node v, kmers[0] = 0.  All
 * three hold n_nodes + 1 entries.  rec_class (host memory, NULL to skip): the class of every record, in the record order of
 * ss_reads_read_back (the records numbered slab after slab).  Nothing depends on the order of the records: file order, binned
 * ASCII and packed slabs give the same direct and node_hits, and the results of a set's shards add up to the whole set's.
 * Synchronous.  Reads the table's index, never its counters.  SS_ERANGE: as ss_reads_select states it.  SS_EINVAL: a NULL argument
 * other than rec_class, min_score == 0, n_nodes outside 1..SS_CLASS_NODES_MAX, a row node above n_nodes, a parent above n_nodes or
 * a cycle, a table and a set on different devices. */
#define SS_CLASS_NODES_MAX 65535
int ss_reads_classify(const ss_db *db, const ss_reads *r, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent,
                      uint32_t min_score, uint64_t *direct, uint64_t *node_hits, uint64_t *kmers, uint32_t *rec_class);
int ss_reads_classify_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* the records whose class came from a tie (score >= min_score) in the calling thread's last ss_reads_classify */
int ss_reads_classify_ties(uint64_t *n);
/* The records of chosen classes as NEW resident sets (`--extract_class`): one classification of the set, exactly that of
 * ss_reads_classify for the same row_node, n_nodes, parent and min_score, and one set per entry of clades[] (host memory):
 *   clades[i] == 0:              out[i] holds the non-empty records of class 0 (unclassified)
 *   clades[i] == v, 1..n_nodes:  out[i] holds the records whose class is v or a descendant of v -- the reads that the sum of
 *                                direct[] over v's subtree counts; a record of class 0 is in no such clade
 * The same clade may be listed twice: each entry gets its own set.  An empty record is never selected.  Every out[i] has the layout
 * of ss_reads_select's *out: one ASCII, unbinned slab, each record's bytes and '\n', the block padded with '\n', letters from a
 * packed slab as ss_reads_read_back writes them, n_records and n_bases of ss_reads_info exact, the order unspecified; nothing
 * selected: a valid set of 0 records.  ss_reads_read_back, ss_scan_reads, ss_reads_support and ss_reads_order work on each set, and
 * the caller destroys each.  direct, node_hits and kmers, each NULL or [n_nodes + 1], are what ss_reads_classify returns, and
 * ss_reads_classify_ties reports this call's ties too.  The classes stay on the device, and the set is classified once however
 * many clades are listed.  Synchronous.  Reads the table's index, never its counters.  SS_ERANGE: as ss_reads_select states it.
 * SS_EINVAL: as ss_reads_classify states it (but direct, node_hits and kmers may be NULL), and clades or out NULL, n_clades
 * outside 1..SS_SELECT_CLADES_MAX, a clade above n_nodes.  On any error every set made so far is destroyed and every out[i] is
 * NULL. */
#define SS_SELECT_CLADES_MAX 64
int ss_reads_select_class(const ss_db *db, const ss_reads *r, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent,
                          uint32_t min_score, const uint32_t *clades, uint32_t n_clades, ss_reads **out /* [n_clades] */,
                          uint64_t *direct, uint64_t *node_hits, uint64_t *kmers /* each NULL, or [n_nodes + 1] */);
int ss_reads_select_class_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* Every record of a resident set assigned to the SET of called strains that explain it best (`--classify_strains`); a record and a
 * hit are those of ss_reads_support.  The caller numbers the called strains 1..n_strains.  row_sets[i], i < the table's rows (host
 * memory), is the row's MASK: bit j - 1 is set when strain j has the row's k-mer.  Rows that share a slot (the same k-mer listed
 * twice) keep their common mask; where they disagree the k-mer has mask 0.
 *   h[j]   = the record's hits whose k-mer's mask has bit j - 1;  h0 = its hits whose k-mer has mask 0
 *   score  = the largest h[j]
 *   set    = { j : h[j] == score } when score >= min_score and score > 0, the empty set otherwise; one strain: a UNIQUE
 *            assignment, several: a TIE, none: unassigned
 * unique[j], j in 1..n_strains: records whose set is {j}; unique[0]: records with the empty set.  tied[j]: records with j in a set
 * of two or more; tied[0]: records with such a set, so sum(unique) + tied[0] = the set's non-empty records.  strain_hits[j] = the
 * sum of h[j] over all records, strain_hits[0] that of h0.  kmers[j]: the distinct k-mers (slots) whose mask has bit j - 1,
 * kmers[0] = 0.  All four hold n_strains + 1 entries.  set_reads (NULL to skip): [1 << n_strains], set_reads[m] = records whose set
 * is the mask m, so set_reads[0] = unique[0] and set_reads[1 << (j-1)] = unique[j].  rec_set / rec_score (host memory, NULL to
 * skip): the set and the score of every record -- the score also where it is below min_score -- in the record order of
 * ss_reads_read_back.  When every mask has at most one bit, h[j] is label j's hits of ss_reads_support_labeled.  Nothing depends on
 * the order of the records: file order, binned ASCII and packed slabs give the same totals, and the results of a set's shards add
 * up to the whole set's.  Synchronous.  Reads the table's index, never its counters.  SS_ERANGE: as ss_reads_select states it.
 * SS_EINVAL: a NULL argument other than set_reads, rec_set and rec_score; min_score == 0; n_strains outside 1..SS_STRAIN_SET_MAX;
 * a row mask with a bit at or above n_strains; a table and a set on different devices. */
#define SS_STRAIN_SET_MAX 16
int ss_reads_classify_strains(const ss_db *db, const ss_reads *r, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score,
                              uint64_t *unique, uint64_t *tied, uint64_t *strain_hits, uint64_t *kmers /* each [n_strains + 1] */,
                              uint64_t *set_reads, uint16_t *rec_set, uint32_t *rec_score);
int ss_reads_classify_strains_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* the records with a tie (tied[0]) in the calling thread's last ss_reads_classify_strains or ss_reads_select_strains */
int ss_reads_classify_strains_ties(uint64_t *n);
/* The records of chosen strain sets as NEW resident sets (`--extract_strains`): one classification of the set, exactly that of
 * ss_reads_classify_strains for the same row_sets, n_strains and min_score, and one set per entry i < n_want (host memory):
 *   how[i] == 0:  out[i] holds the records whose set EQUALS the mask want[i]; want[i] == 0: the unassigned records
 *   how[i] == 1:  out[i] holds the records whose set INTERSECTS want[i] (never a record with the empty set)
 * The same entry may be listed twice: each gets its own set.  An empty record is never selected.  Every out[i] has the layout of
 * ss_reads_select's *out, and the caller destroys each.  unique, tied, strain_hits and kmers, each NULL or [n_strains + 1], are
 * what ss_reads_classify_strains returns.  The sets of the records stay on the device, and the set is classified once however
 * many entries are listed.  Synchronous.  Reads the table's index, never its counters.  SS_ERANGE: as ss_reads_select states it.
 * SS_EINVAL: as ss_reads_classify_strains states it (but the four arrays may be NULL), and want, how or out NULL, n_want outside
 * 1..SS_SELECT_STRAINS_MAX, a want[i] with a bit at or above n_strains, a how[i] above 1.  On any error every set made so far is
 * destroyed and every out[i] is NULL. */
#define SS_SELECT_STRAINS_MAX 32
int ss_reads_select_strains(const ss_db *db, const ss_reads *r, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score,
                            const uint16_t *want, const uint8_t *how, uint32_t n_want, ss_reads **out /* [n_want] */,
                            uint64_t *unique, uint64_t *tied, uint64_t *strain_hits, uint64_t *kmers /* each NULL, or [n_strains + 1] */);
int ss_reads_select_strains_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* The set counts of several bootstrap replicates from ONE classification of the set (`--em_strains`): set_reads[j][m] (host memory,
 * [n_replicates][1 << n_strains], j < n_replicates <= SS_SCAN_REPLICATES_MAX) is, bit for bit, what ss_reads_classify_strains
 * returns as set_reads[m] on the set that ss_reads_resample(r, seed, first_replicate + j) returns -- the sum, over the records of r
 * whose set is the mask m, of the weight ss_reads_resample states for (the record, seed, first_replicate + j).  A record's set does
 * not depend on its copies, so nothing is materialised: the records are classified once, their weights are drawn once (sixteen
 * 4-bit fields of one word per record) and one pass adds every weight that is not zero to its replicate's counter of the
 * record's set.  Works on every kind of resident set, as ss_reads_classify_strains does.  Synchronous.  Reads the table's index,
 * never its counters.  SS_ERANGE and SS_EINVAL: as ss_reads_classify_strains states them (set_reads must not be NULL), and
 * SS_EINVAL for n_replicates outside 1..SS_SCAN_REPLICATES_MAX. */
int ss_reads_strain_sets_resampled(const ss_db *db, const ss_reads *r, const uint16_t *row_sets, uint32_t n_strains, uint32_t min_score,
                                   uint64_t seed, uint32_t first_replicate, uint32_t n_replicates,
                                   uint64_t *set_reads /* host, [n_replicates][1 << n_strains] */);
int ss_reads_strain_sets_resampled_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* Read-based strain abundances by EM over the equivalence classes of ss_reads_classify_strains (`--em_strains`), n_vec count
 * vectors in one launch.  masks[s], s < n_sets (host memory): a set of called strains, bit j - 1 for strain j in 1..n_strains;
 * non-zero, distinct.  counts[v][s] (host memory): the reads of vector v whose set is masks[s].  Per vector, in float64, with
 * n_s = counts[v][s] and N = the sum of the n_s (taken in integers):
 *   active    strain j is ACTIVE when some set with n_s > 0 holds j; an inactive strain has rho_j = 0 throughout
 *   start     rho_j = 1 / (the number of active strains)
 *   one iteration, for every set with n_s > 0:  d_s = the sum of rho_i over i in the set, i ascending;  a set with d_s == 0
 *             contributes nothing;  rho'_j = rho_j * (the sum over the sets s that hold j of n_s / d_s) / N
 *             -- that is (1/N) * sum of n_s * rho_j / d_s, with the common factor rho_j taken out of the sum
 *   stopping  after iteration t: when t == max_iter, or when the largest |rho'_j - rho_j| < tol; tol == 0 runs exactly max_iter
 *             iterations.  iters[v] = the iterations run
 *   N == 0    rho = 0 everywhere, iters[v] = 0
 * rho[v][j - 1] = strain j's share of vector v's assigned reads; the rho of a vector sum to 1 up to rounding.  The order in which
 * the device adds the sets' terms is fixed (a strided share per thread, a fixed tree within the wave, the waves in order), so the
 * same input gives the same bits on every run; it is not the ascending order, so rho differs from tests/em_model.py's by the
 * rounding of a sum taken in another order.  No floating-point atomics.  One launch per call, one workgroup per vector, which
 * tests convergence itself; masks and counts stay in LDS up to SS_EM_LDS_SETS sets and are read from global memory in every
 * iteration above.  Synchronous, on the current device.  SS_EINVAL: a NULL argument; n_sets outside 1..65535; n_strains outside
 * 1..SS_STRAIN_SET_MAX; n_vec outside 1..SS_EM_VECTORS_MAX; max_iter == 0; tol negative or NaN; a mask that is zero, listed twice
 * or has a bit at or above n_strains. */
#define SS_EM_VECTORS_MAX 1024
#define SS_EM_LDS_SETS 6144
int ss_em_strain_sets(const uint64_t *counts /* [n_vec][n_sets] */, const uint16_t *masks /* [n_sets] */, uint32_t n_sets, uint32_t n_strains,
                      uint32_t n_vec, uint32_t max_iter, double tol, double *rho /* [n_vec][n_strains] */, uint32_t *iters /* [n_vec] */);
int ss_em_strain_sets_calls(uint64_t *n);  /* calls so far in this process (diagnostics; "flag off = not run") */
/* The runs of missing k-mers inside the records of a resident set, against the k-mers of the called strains (`--divergence`): how
 * far the sample's organism is from the nearest called strain, without an alignment.  A record and a hit are those of
 * ss_reads_support.  row_called[i], i < the table's rows (host memory): non-zero = a called strain has the row's k-mer; NULL: every
 * row is called.  A slot (a distinct k-mer) is CALLED when ANY of its rows is: a k-mer listed twice is one k-mer and takes the union
 * of its rows -- not the agree-or-zero rule of the label and mask folds.  For a record of n bytes:
 *   base      a byte that is one of ACGTacgt
 *   window p  0 <= p <= n - k; VALID when bytes p .. p + k - 1 are all bases.  The state of a valid window: C, its k-mer is a called
 *             slot; T, its k-mer is in the table but not called; X otherwise.  C and T together are the record's hits.  An invalid
 *             window has state I.
 *   counts    hits_called, hits_cluster, misses = the record's C, T, X; windows = their sum
 *   assessed  hits_called >= min_hits; only assessed records add to the totals below
 *   gap       a maximal run of windows [p, p + g) that are all T or X, with window p - 1 and window p + g both existing and both C.
 *             An I window is never inside a gap and never flanks one: no gap spans an N, a masked base or the joint of a pair.
 *             IN-CLUSTER: every window of it is T.  Length classes: gap_lt g < k - 1; gap_km1 g = k - 1 (a deleted base);
 *             gap_k g = k (a substituted base); gap_k_2k k < g < 2 k (an insertion of g - k + 1 bases, two differences less than
 *             k apart); gap_ge2k g >= 2 k
 *   site      a gap with k - 1 <= g < 2 k that is not in-cluster
 *   stretch   a maximal run of valid windows; for one that holds a C, first / last = its first / last C window
 *   detectable  the sum over the record's stretches with a C of max(0, last - first - k): a substitution at base b of a fully
 *             matching stretch gives a flanked gap exactly when first + k <= b <= last - 1.  A clean 150-base read at k = 31: 88.
 * out[]: [0] records (all non-empty records of the set), then summed over the assessed records [1] assessed, [2] windows,
 * [3] hits_called, [4] hits_cluster, [5] misses, [6] gap_lt, [7] gap_km1, [8] gap_k, [9] gap_k_2k, [10] gap_ge2k,
 * [11] gaps_in_cluster, [12] sites, [13] reads_with_sites, [14] detectable; [15] kmers = the occupied slots of the table,
 * [16] kmers_called = the called ones; [17] the records of more than 4095 bytes, which take the call's general pass
 * (diagnostics).  rec_out (host memory, NULL to skip): four values per record -- hits_called, its gaps of all classes, its sites,
 * its detectable -- in the record order of ss_reads_read_back, for the records that are not assessed too.  Nothing depends on the
 * order of the records: file order, binned ASCII and packed slabs give the same totals, and the totals of a set's shards ([0]..[14],
 * [17]) add up to the whole set's.  Synchronous.  Reads the table's index, never its counters.  SS_ERANGE: as ss_reads_select states
 * it.  SS_EINVAL: db, r or out NULL; min_hits == 0; a table and a set on different devices. */
#define SS_GAPS_OUT 18
int ss_reads_gaps(const ss_db *db, const ss_reads *r, const uint8_t *row_called /* NULL: every row */, uint32_t min_hits,
                  uint64_t out[SS_GAPS_OUT], uint32_t *rec_out /* NULL, or [records][4] */);
int ss_reads_gaps_calls(uint64_t *n);      /* calls so far in this process (diagnostics; "flag off = not run") */
/* Read PAIRS as the records of a resident set (`--pairs`, ss_pairs.hip).  A resident set keeps no pair map, and every call above
 * decides per record from the record's bytes alone: on a set whose records are the pairs they all work on fragments, unchanged.
 * The join rule: record i of the result is  line1[i] + 'N' + line2[i] + '\n'.  'N' ends a k-mer window, so no k-mer spans the
 * joint and the fragment's hits against any table are the two mates' hits added up.
 * ss_reads_join_pairs_dev: flat1_dev / flat2_dev are flat base blocks on the device as ss_fastx_to_flat writes them, exact
 *   length, every record followed by one '\n'.  A LINE is the bytes between two consecutive '\n' (from the block's start for
 *   the first) and may be empty -- a record without bases, which ss_fastx_to_flat emits and counts -- so lines are numbered over
 *   EVERY '\n': an empty record in one file does not shift the pairing.  The 'N' is written even where a mate is empty (two empty
 *   mates: the record "N"), so n_records = the lines of either block, and the bytes of the lines are copied as they are (lower
 *   case, IUPAC codes, '\r').  Joined record i begins at byte start1[i] + start2[i] and the result holds exactly n1 + n2 bytes:
 *   the 'N' takes the place of mate 1's '\n', no prefix sum is needed.
 *   order == 0: one ASCII, unbinned slab in the layout of ss_reads_select's *out, padded with '\n', in LINE ORDER;
 *   n_records and n_bases of ss_reads_info exact.  order != 0: the same set after ss_reads_order (order unspecified, packed
 *   where the records allow it: 150 + 1 + 150 bases of A C G T N do).  Two empty blocks: a valid set of 0 records.
 *   Synchronous; has no cut record.  SS_EIO: the blocks hold different numbers of lines.  SS_EINVAL: a NULL argument, a non-empty
 *   block whose last byte is not '\n'.  SS_ERANGE: more than 2^32 - 1 lines.  On any error *out is NULL.
 * ss_reads_load_pairs: each file as ONE flat block in file order on the device (a thread per file; FASTA and FASTQ, plain or
 *   gzip, four-line and wrapped, CRLF; the base-quality mask with the grammar of ss_fastx_to_flat), then the join.
 *   ss_reads_load is not involved.  SS_EINVAL: a BAM or CRAM input, a NULL or empty path.  SS_EIO: an unreadable file, unequal
 *   record counts. */
int ss_reads_join_pairs_dev(const void *flat1_dev, uint64_t n1, const void *flat2_dev, uint64_t n2, int order, ss_reads **out);
int ss_reads_join_pairs_calls(uint64_t *n);    /* joins so far in this process (diagnostics; "flag off = not run") */
int ss_reads_load_pairs(const char *path1, const char *path2, int order, ss_reads **out);
/* The per-read table of `--read_calls` (ss_calls.hip, ss_pairs.hip, ss_extract.hip): which record went where, and on what evidence.
 * ss_reads_calls: ss_reads_classify for the same arguments -- a record, a hit, h[v], score and class are exactly its -- with the
 *   results per record.  `records` is the set's non-empty records, numbered in the record order of ss_reads_read_back.
 *   rec_class[i]: the class of record i.  rec_score[i]: the largest score(v) of record i, 0 when no hit has a node; reported also
 *   where it lies below min_score (ss_bam_tag_stream's sc).  The HIT LIST of record i is entries rec_first[i] .. rec_first[i + 1] - 1
 *   of list_node / list_hits: every node v >= 1 with h[v] > 0, in ascending v, list_hits = h[v] (32 bits); hits of k-mers without
 *   a node are not listed (they stay in node_hits[0]).  rec_first holds records + 1 entries, rec_first[records] == *n_list.
 *   cap: the entries list_node / list_hits hold; both may be NULL with cap == 0.  That, or any cap < *n_list, returns SS_ERANGE
 *   with *n_list set, and nothing else is to be used: the caller comes again with room for *n_list.  direct, node_hits, kmers (each
 *   NULL or [n_nodes + 1]) and ss_reads_classify_ties are what ss_reads_classify gives.  Works on any set: file order, binned
 *   ASCII, packed, several slabs (the lists then follow that set's record order).  Synchronous.  Errors otherwise as
 *   ss_reads_classify states them; SS_EINVAL also for a NULL rec_class, rec_score, rec_first or n_list.
 * ss_reads_load_ordered: ONE FASTA/FASTQ file as one ASCII, unbinned slab in FILE ORDER (plain or gzip, four-line and wrapped,
 *   CRLF; the base-quality mask with the grammar of ss_fastx_to_flat): record i of the set is the i-th record of the file that
 *   has a sequence.  ss_reads_load is not involved.  SS_EINVAL: a BAM or CRAM input, a NULL or empty path.  SS_EIO: an unreadable
 *   file.
 * ss_read_calls_write (host; no device needed): walks the n_in (1 or 2) input files with the record grammar of ss_fastx_to_flat,
 *   as ss_extract_write does, and writes to out_paths[f] the header  name TAB node TAB score TAB length TAB hits  and one such
 *   line per record of input f, in file order.  name: the header line behind its first character up to the first space, tab, CR
 *   or LF (may be empty).  node: node_value[class] ([n_nodes + 1]; the commands pass the ids of read_classes.tsv and -1 for class
 *   0).  length: the record's sequence characters (CR not counted).  hits: `id:h` items, id = node_value[v], separated by one
 *   space, in list order; `-` for an empty list.  n_in == 1: the i-th record of the file that has a sequence takes entry i; a
 *   record without one has no record in the set, is written as  name -1 0 0 -  and takes no entry.  n_in == 2 (a set of joined
 *   pairs in line order): record j of BOTH files takes entry j -- a fragment is never empty --, length is the mate's own, node,
 *   score and hits are the fragment's.  counters[0] records read, [1] lines written (the header apart), [2] lines of class != 0,
 *   [3] records with an empty sequence.  One file is shared over up to min(16, SS_HOST_THREADS or the CPUs this process may use)
 *   host threads by the chunks the ordered load parsed it in; the output does not depend on their number.  SS_EIO: the walk does not end at exactly n_records, the two files differ in records, an
 *   unreadable input, an output that cannot be written.  SS_EINVAL: a BAM or CRAM input, a bad argument, offsets that do not
 *   ascend, a class or a listed node outside 1..n_nodes (class: 0..n_nodes).  On any error no output file is left behind (the
 *   text goes to <name>.tmp, renamed at the end). */
int ss_reads_calls(const ss_db *db, const ss_reads *r, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent,
                   uint32_t min_score, uint32_t *rec_class, uint32_t *rec_score, uint64_t *rec_first /* [records + 1] */,
                   uint32_t *list_node, uint32_t *list_hits, uint64_t cap, uint64_t *n_list,
                   uint64_t *direct, uint64_t *node_hits, uint64_t *kmers /* each NULL, or [n_nodes + 1] */);
int ss_reads_calls_calls(uint64_t *n);     /* calls so far in this process (diagnostics; "flag off = not run") */
int ss_reads_load_ordered(const char *path, ss_reads **out);
int ss_read_calls_write(const char *const *in_paths, int n_in /* 1, or 2 for a joined pair set */, const char *const *out_paths,
                        uint64_t n_records, const uint32_t *rec_class, const uint32_t *rec_score, const uint64_t *rec_first,
                        const uint32_t *list_node, const uint32_t *list_hits, const int64_t *node_value /* [n_nodes + 1] */,
                        uint32_t n_nodes, uint64_t counters[4]);

/* --------------------------------------------------------------------------------------------
 * Extracted reads on the host (ss_extract.hip; no device needed).  What ss_reads_select chose is carried back to the input
 * files BY CONTENT: a record is named by a 128-bit digest of its flat form -- two independent 64-bit hashes over its bytes and
 * its length: FNV-1a (64-bit) and a multiply-rotate hash over 8-byte words with a splitmix64 finish, each closed with the
 * length.  A record that was not selected is written only if BOTH hashes collide with a selected one's: a false positive needs
 * a 128-bit collision.  Reads with the same flat form share a digest and a fate.
 * ss_flat_record_keys: keys[2 i], keys[2 i + 1] = the digest of the i-th non-empty record ('\n'-separated) of a flat block;
 *   *n_records = how many there are; SS_ERANGE (and *n_records set) when cap (in records) is too small; keys = NULL counts.
 *   The flat block is taken as the loader made it: with the base-quality mask on, it is the masked form.
 * ss_extract_write: reads the n_in (1 or 2) input files again -- plain text mapped, .gz through the host inflater -- walks them
 *   record by record with the grammar of ss_fastx_to_flat (four-line and multi-line FASTQ, FASTA of any wrapping, CRLF; the
 *   base-quality mask applied), and writes the ORIGINAL TEXT of every record whose flat form's digest is among the n_keys
 *   digests of `keys`, byte for byte, to out_paths[i].  Two inputs are walked in lockstep and record i of both files is
 *   written when EITHER mate is selected.  A record with an empty sequence has no digest and is never selected (in a pair it
 *   goes along with a selected mate, so that the two files stay in step).
 *   counters[0] records read, all inputs together, [1] records written, all outputs together, [2] pairs written because of
 *   mate 1 only, [3] because of mate 2 only.  SS_EIO: an unreadable input, unequal record counts; SS_EINVAL: a BAM or CRAM input, a bad
 *   argument.  On any error no output file is left behind (the text goes to <name>.tmp, renamed at the end).
 * ss_extract_write_pairs: the same walk over exactly two inputs (n_in == 2, two outputs) for a selection made on a set of
 *   joined pairs (ss_reads_join_pairs_dev): pair i is named by the digest of  flat1[i] + 'N' + flat2[i]  -- what
 *   ss_flat_record_keys gives for the joined set's records -- and BOTH records of the pair are written, original text byte for
 *   byte, when that digest is among `keys`.  An empty mate is not special: the fragment is never empty.  counters[0] records
 *   read, [1] records written, [2] pairs written, [3] 0.  Errors and clean-up as ss_extract_write's.
 * ------------------------------------------------------------------------------------------ */
int ss_flat_record_keys(const char *flat, uint64_t len, uint64_t *keys, uint64_t cap, uint64_t *n_records);
int ss_extract_write(const char *const *in_paths, int n_in, const uint64_t *keys, uint64_t n_keys,
                     const char *const *out_paths, uint64_t counters[4]);
int ss_extract_write_pairs(const char *const *in_paths, int n_in, const uint64_t *keys, uint64_t n_keys,
                           const char *const *out_paths, uint64_t counters[4]);

/* --------------------------------------------------------------------------------------------
 * Host FASTA/FASTQ -> flat base block (what jellyfish's sequence parser feeds its counter).
 * out must hold at least len + 2 bytes.  Used by ss_scan_files and exposed for callers that
 * shard reads themselves (multi-GPU).
 * ------------------------------------------------------------------------------------------ */
int ss_fastx_to_flat(const char *text, uint64_t len, char *out, uint64_t *out_len, uint64_t *n_records);

/* --------------------------------------------------------------------------------------------
 * BAM input.  A path is a BAM when its first gzip member inflates to bytes that begin with "BAM\1" (or the file itself
 * is such an uncompressed stream); ss_reads_load and ss_scan_files(_shard) decode it whole -- inflated and decoded on the
 * device first (files of 1 MB and more, unless SS_GZ_GPU=0 or policy 2), on the host for what the device declines.  The
 * reads are those of a default `samtools fastq`: secondary (0x100) and supplementary (0x800) records and records without
 * bases are skipped, a 0x10 record is reverse-complemented, each 4-bit code becomes its letter of "=ACMGRSVTWYHKDBN"; the
 * flat block is each kept record's letters and '\n'.  Under sharding a rank keeps the blocks of 4096 KEPT records
 * b = rank, rank + world, ...  A damaged stream (a member's CRC or length, a record that breaks the layout or runs past the
 * end, no "BAM\1") makes the call return SS_EIO with nothing loaded; a CRAM file is refused with SS_EINVAL.
 * ------------------------------------------------------------------------------------------ */
/* What a path holds: *kind = 0 anything else (FASTA/FASTQ, plain or gzip, or unreadable), 1 a gzip'ed (BGZF) BAM, 2 an
 * uncompressed BAM stream, 3 a CRAM file.  Reads the first 64 KB.  Host only, any thread. */
int ss_input_kind(const char *path, int *kind);
/* The host decoder over an inflated BAM stream of n bytes (from "BAM\1"): the flat block of this rank's kept records ->
 * out (out = NULL: only *out_len), *n_records = this rank's kept records.  SS_ERANGE when cap < *out_len, SS_EIO when the
 * stream is damaged (nothing written is to be used).  Host only, any thread; the buffers stay the caller's. */
int ss_bam_decode(const void *stream, uint64_t n, int shard_rank, int shard_world, char *out, uint64_t cap, uint64_t *out_len,
                  uint64_t *n_records);
/* BAM inputs so far in this process: out[0] files decoded on the device, out[1] files decoded on the host, out[2] records
 * kept, out[3] records skipped (over all ranks' shares: every rank walks the whole stream).  Any thread. */
int ss_bam_counters(uint64_t out[4]);
/* --------------------------------------------------------------------------------------------
 * Extracted reads from a BAM (`-x` / `--by_strain` on a BAM sample; ss_bam_extract.hip).  The output holds, in file order and
 * byte for byte (block_size, name, flags, CIGAR, bases, qualities, every tag), every KEPT record of a selected TEMPLATE.  Kept is
 * the loader's rule: neither 0x100 nor 0x800, l_seq != 0; a record that is not kept is never written, whatever its name.  A kept
 * record is selected when the flat form the loader makes of it (reverse-complemented for 0x10, under the base-quality mask) has
 * at least min_hits hits against the table, a hit being that of ss_reads_support -- with row_labels the hits of `label`, as
 * ss_reads_select_labeled counts them.  A kept record is written when it is selected or when its read name (the bytes before the
 * first NUL) equals that of a selected record of the same stream: mates, wherever they lie.  Names are compared through a 128-bit
 * digest of their bytes and length (two independent 64-bit hashes): a true match is never missed, a record is written without one
 * only on a 128-bit collision.  Needs the stream and the open table only -- no resident set; records of any length.
 * ss_bam_select: stream = an inflated BAM stream in HOST memory (from "BAM\1").  row_labels == NULL: all hits; else as
 *   ss_reads_select_labeled.  out: the written records, concatenated, in file order (no header); *out_len their bytes.
 *   counters: [0] records of the stream, [1] kept, [2] selected by hits, [3] written.  SS_ERANGE with *out_len and the counters
 *   set when cap is too small; SS_ERANGE for a flat table (k below 17); SS_EIO a damaged stream; SS_EINVAL as
 *   ss_reads_select(_labeled) (a NULL argument, min_hits == 0, labels out of range).
 * ss_bam_extract: one BAM file (BGZF, plain gzip or uncompressed) -> out_path, a BGZF BAM: the input's header from "BAM\1" to
 *   the first record, byte for byte, then those records.  The file is inflated on the device where ss_reads_load would do that
 *   (1 MB and more, not under SS_GZ_GPU=0), else on the host and uploaded; ss_bam_counters counts it under out[0] or out[1]
 *   accordingly.  Written to <out_path>.tmp and renamed at the end; nothing is left on an error.  Members are compressed at zlib
 *   level 1 (SS_BAM_OUT_LEVEL=0..9 changes it): the file step of ss_bam_out.hip, which ss_bam_tag_file takes too.  SS_EINVAL also
 *   for an input that is not a BAM.
 * ss_bgzf_write (host only; ss_bam_out.hip): head's bytes, then body's, as BGZF members of at most 0xff00 stream bytes each -- the "BC" extra
 *   field, raw deflate at `level` (0..9), CRC-32, ISIZE -- and the 28-byte EOF block; a member never holds bytes of both.  The
 *   members are compressed on up to min(16, SS_HOST_THREADS or the CPUs this process may use) threads.  SS_EIO (and no file)
 *   when path cannot be written.
 * ss_bam_extract_calls: calls of ss_bam_select and ss_bam_extract so far in this process ("flag off = not run").
 * ss_bam_extract_timing: the last successful ss_bam_extract, host clock around its synchronised steps (ms): out[0] stream on the
 *   device (inflate, or host inflate + upload), [1] walk + decode, [2] hits, [3] join, [4] gather, [5] download, [6] compress +
 *   write, [7] the whole call.
 * ------------------------------------------------------------------------------------------ */
int ss_bam_select(const void *stream, uint64_t n, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                  uint32_t min_hits, void *out, uint64_t cap, uint64_t *out_len, uint64_t counters[4]);
int ss_bam_extract(const char *in_path, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                   uint32_t min_hits, const char *out_path, uint64_t counters[4]);
int ss_bgzf_write(const char *path, const void *head, uint64_t head_n, const void *body, uint64_t body_n, int level);
int ss_bam_extract_calls(uint64_t *n);
int ss_bam_extract_timing(double out[8]);
/* --------------------------------------------------------------------------------------------
 * Read pairs from a BAM (`--pairs` on a BAM sample; ss_bam_pairs.hip).  A paired BAM holds both mates in one stream, anywhere.
 * The rule (tests/bam_pairs_model.py restates it):
 *   KEPT is the loader's rule (neither 0x100 nor 0x800, l_seq != 0); flat(r) is the loader's form of kept record r (reverse-
 *   complemented for 0x10, letters, the base-quality mask); the NAME is the bytes of read_name before the first NUL, compared by
 *   BOTH 64-bit hashes of the digest ss_bam_select uses.  Records that are not kept never count.
 *   A kept record with 0x1 clear is a SINGLE and takes no part in the name join.  A kept record with 0x1 set has ROLE 1 (0x40 set,
 *   0x80 clear), ROLE 2 (0x80 set, 0x40 clear) or ROLE 0.  The 0x1 records of one name form a group: one record = an ORPHAN; two
 *   records of roles {1, 2} = a PAIR; anything else (three and more, two of one role, a role 0 that shares its name) = a
 *   VIOLATION: the call returns SS_EIO, builds nothing and still fills the counters.
 *   Fragments: a pair gives flat(m1) 'N' flat(m2) '\n'; an orphan of role 2 gives 'N' flat '\n'; an orphan of role 0 or 1 and a
 *   single give flat 'N' '\n'.  No k-mer spans the N: the hits of the fragments add up to those of the kept records.  The set
 *   holds (flat_len - kept) + 2 x fragments bytes before padding; fragments stand in ascending stream position of each one's
 *   earlier record.  One rank only.
 * counters[6]: records, kept, pairs, orphans, singles, records in violating groups.
 * ss_bam_mates: stream = an inflated BAM stream in HOST memory.  mate[r] (cap >= records, else SS_ERANGE with the counters set) =
 *   the mate's record index, 0xFFFFFFFE no mate (single, orphan, member of a violating group), 0xFFFFFFFF not kept.  mate[] is
 *   filled with a violation too (SS_EIO and counters[5] != 0); SS_EIO with counters[5] == 0 is a damaged stream.
 * ss_reads_join_pairs_bam: the fragments of such a stream as a resident set.  order == 0: one ASCII slab in the layout of
 *   ss_reads_select's *out; order != 0: the same set after ss_reads_order.  A stream without kept records: a valid set of 0
 *   records.  On any error *out is NULL.
 * ss_reads_load_pairs_bam: the same from one BAM file, brought to the device the way ss_bam_extract brings it.  SS_EINVAL: not a
 *   BAM.  Both count under ss_reads_join_pairs_calls.  The file is inflated again beside ss_reads_load's own pass.
 * ss_bam_select_pairs / ss_bam_extract_pairs: ss_bam_select / ss_bam_extract by FRAGMENT: a kept record is written iff its own hits
 *   plus its mate's reach min_hits; there is no further name join.  counters: [0] records, [1] kept, [2] fragments selected, [3]
 *   records written.  A violation: SS_EIO and no file.
 * ss_bam_pairs_timing: the last successful ss_reads_load_pairs_bam, host clock around its synchronised steps (ms): out[0] stream
 *   on the device, [1] walk + decode, [2] keys, [3] sort, [4] link, [5] lengths + scan, [6] join (and the ordering pass when
 *   asked for), [7] the whole call.
 * ------------------------------------------------------------------------------------------ */
int ss_bam_mates(const void *stream, uint64_t n, uint32_t *mate, uint64_t cap, uint64_t counters[6]);
int ss_reads_join_pairs_bam(const void *stream, uint64_t n, int order, ss_reads **out, uint64_t counters[6]);
int ss_reads_load_pairs_bam(const char *path, int order, ss_reads **out, uint64_t counters[6]);
int ss_bam_select_pairs(const void *stream, uint64_t n, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                        uint32_t min_hits, void *out, uint64_t cap, uint64_t *out_len, uint64_t counters[4]);
int ss_bam_extract_pairs(const char *in_path, const ss_db *db, const uint8_t *row_labels, uint32_t n_labels, uint32_t label,
                         uint32_t min_hits, const char *out_path, uint64_t counters[4]);
int ss_bam_pairs_timing(double out[8]);
/* --------------------------------------------------------------------------------------------
 * Tagged BAM (`--tag_bam`; ss_bam_tag.hip): a BAM stream written back with the class of every read as two aux tags.  The rule
 * (tests/bam_tag_model.py restates it):
 *   KEPT is the loader's rule (neither 0x100 nor 0x800, l_seq != 0); flat(r) is the loader's form of kept record r (reverse-
 *   complemented for 0x10, codes turned to letters, the base-quality mask).  The CLASS of kept record r is that of
 *   ss_reads_classify on flat(r) for the same row_node, n_nodes, parent and min_score; its SCORE is the largest score(v) of the
 *   record, 0 when no hit has a node -- reported also where it is below min_score and the class is therefore 0.
 *   The output body is EVERY record of the stream in file order.  A record that is not kept is copied byte for byte.  A kept
 *   record is copied byte for byte with SS_BAM_TAG_BYTES = 14 bytes appended behind its last aux field, and its block_size field
 *   is raised by 14:   t0 t1 'i' <int32 LE node_value[class]>   t2 t3 'i' <int32 LE score>
 *   node_value[0..n_nodes] (host memory) is the caller's: the CLI passes the node ids of read_classes.tsv and -1 for class 0.
 *   tags is four bytes, t0 t1 t2 t3; the CLI passes "snsc" (lower-case tags are reserved for end users by the SAM specification).
 *   The body holds (n - hdr_end) + 14 x kept bytes; kept record r moves to rec[r] - hdr_end + 14 x (the kept records before it),
 *   and so does a record that is not kept.
 *   pairs != 0: the mates are linked and the fragments built as "Read pairs from a BAM" states (a pair is flat(m1) N flat(m2),
 *   orphans and singles stand alone), from the same stream inside the call -- no second inflation; the fragments are classified and
 *   BOTH records of a pair receive the fragment's class and score.  A violating name group: SS_EIO and no output.
 *   Existing tags.  The aux fields of every kept record are walked by field -- tag[2], type[1], then the value: A c C 1 byte, s S
 *   2, i I f 4, Z H up to and with a NUL, B subtype[1] count[4] and count x size(subtype) bytes.  A kept record that already has a
 *   field named t0t1 or t2t3 would make an invalid BAM: SS_EIO, nothing is written, counters[3] = the number of such records.  A
 *   byte pair that merely occurs inside a value is no field.  A field of unknown type, or one that runs past the record's end, is a
 *   damaged stream: SS_EIO with counters[3] == 0 (also when other records bear a tag).  Records that are not kept are not walked.
 * counters: [0] records, [1] kept == tagged, [2] kept records of a class != 0, [3] kept records that already bear one of the tags,
 *   [4] fragments (== kept when pairs == 0), [5] fragments whose class came from a tie.  direct, node_hits, kmers: each NULL or
 *   [n_nodes + 1], what ss_reads_classify returns for the same reads (under pairs: for the fragments).
 * ss_bam_tag_stream: stream = an inflated BAM stream in HOST memory (from "BAM\1"); out: the body (no header), *out_len its bytes.
 * ss_bam_tag_file: one BAM file (BGZF, plain gzip or uncompressed), brought to the device the way ss_bam_extract brings it ->
 *   out_path, a BGZF BAM through the same file step (ss_bam_out.hip, ss_bgzf_write): the input's header from "BAM\1" to the first
 *   record, byte for byte, then the body; zlib level 1 (SS_BAM_OUT_LEVEL=0..9 changes it); written to <out_path>.tmp and renamed;
 *   nothing is left on any error.
 * ss_bam_tag_calls: calls of the two so far in this process ("flag off = not run").
 * ss_bam_tag_timing: the last successful ss_bam_tag_file, host clock around its synchronised steps (ms): out[0] stream on the
 *   device, [1] walk + decode, [2] mate link + join, [3] classify, [4] tag check + copy, [5] download, [6] compress + write, [7] the
 *   whole call.
 * SS_EINVAL: a NULL argument other than direct, node_hits and kmers; min_score == 0; n_nodes outside 1..SS_CLASS_NODES_MAX, a row
 *   node or a parent above n_nodes, a cycle; a tag that is not [A-Za-z][A-Za-z0-9], two equal tags; a file that is not a BAM.
 * SS_ERANGE: a flat table (k below 17); with *out_len and the counters set when cap is too small.  SS_EIO: as the rule states (the
 *   counters are set), and a damaged stream.
 * ------------------------------------------------------------------------------------------ */
#define SS_BAM_TAG_BYTES 14
int ss_bam_tag_stream(const void *stream, uint64_t n, const ss_db *db, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent,
                      uint32_t min_score, const int32_t *node_value /* [n_nodes + 1] */, const char tags[4], int pairs, void *out,
                      uint64_t cap, uint64_t *out_len, uint64_t counters[6], uint64_t *direct, uint64_t *node_hits,
                      uint64_t *kmers /* each NULL, or [n_nodes + 1] */);
int ss_bam_tag_file(const char *in_path, const ss_db *db, const uint32_t *row_node, uint32_t n_nodes, const uint32_t *parent,
                    uint32_t min_score, const int32_t *node_value /* [n_nodes + 1] */, const char tags[4], int pairs,
                    const char *out_path, uint64_t counters[6], uint64_t *direct, uint64_t *node_hits,
                    uint64_t *kmers /* each NULL, or [n_nodes + 1] */);
int ss_bam_tag_calls(uint64_t *n);
int ss_bam_tag_timing(double out[8]);
/* The base-quality mask (jellyfish count -Q; off by default).  With a threshold q in 1..93 every decoder that turns a file or a
 * text into bases -- ss_reads_load, ss_scan_files, ss_scan_files_shard, ss_reader_open / ss_reader_next (a reader keeps the
 * threshold it was opened under), ss_fastx_to_flat, ss_bam_decode -- writes 'N' for a base whose quality is below it:
 *   FASTQ  the i-th sequence character of a record, when the i-th quality character the record grammar consumes for it has a
 *          byte value < 33 + q (line breaks count on neither side): `jellyfish count -Q chr(33 + q)`;
 *   FASTA  untouched;
 *   BAM    base i when qual[i] < q, in the stored order (before a 0x10 record is turned round); a record without qualities
 *          (qual[0] == 0xFF) is NOT masked and is counted in ss_mask_counters.
 * Record count, record lengths and order never change.  One process-wide setting: SS_ERANGE outside 0..93, 0 = off.  Set it
 * before the load it is meant for, not while one runs.  ss_mask_counters: out[0] sequence characters masked (those whose quality
 * was below the threshold, an 'N' among them counted too), out[1] BAM records that carried no qualities while the mask was on;
 * cumulative per process, over this process's share of a sharded input.  Host only, any thread. */
int ss_set_min_base_qual(int q);
int ss_get_min_base_qual(void);
int ss_mask_counters(uint64_t out[2]);
typedef struct ss_reader ss_reader;
int ss_reader_open(const char *const *paths, int n_paths, ss_reader **out);
/* a record longer than the caller's buffer is cut and its last `overlap` bases are repeated at
 * the start of the next block; must be k-1 for exact counts (default 30) */
int ss_reader_set_overlap(ss_reader *r, int overlap);
/* fills `out` with whole records up to cap bytes; *out_len == 0 at end of input */
int ss_reader_next(ss_reader *r, char *out, uint64_t cap, uint64_t *out_len, uint64_t *n_records);
int ss_reader_close(ss_reader *r);

/* --------------------------------------------------------------------------------------------
 * Per-node reductions = match_node + del_outlier for every tree node at once
 * (library/identify.py:106-127; identify_low_depth.py:77-101).
 * Node lists are the files <db>/kmers/<id> (0-based rows of kmer.fa), de-duplicated by the
 * caller (the reference turns them into a set, identify.py:118).
 * For node j with rows R_j:
 *   length  = |{r in R_j : row_valid[r]}|                      (identify.py:119,127)
 *   n_pos   = |{r : valid, counts[r] > 0}|                      (:121-124)
 *   median2 = 2 * np.median(profile)  (exact integer)           (:107)
 *   n_kept / sum_kept = size / sum of {c : c < 100*median}      (:106-112)
 * ------------------------------------------------------------------------------------------ */
typedef struct ss_nodes ss_nodes;
typedef struct {
    uint32_t length;
    uint32_t n_pos;
    uint32_t n_kept;
    uint32_t reserved;
    uint64_t sum_kept;
    uint64_t median2;
} ss_node_stat;
int ss_nodes_create(const uint32_t *rows, const uint64_t *offsets, uint32_t n_nodes, ss_nodes **out);
int ss_nodes_destroy(ss_nodes *ns);
int ss_nodes_reduce_dev(const ss_nodes *ns, const uint32_t *counts_rows_dev, const uint8_t *row_valid_dev,
                        ss_node_stat *stats_dev, void *stream);
int ss_nodes_reduce(const ss_nodes *ns, const ss_db *db, ss_node_stat *stats /* host, n_nodes */);
/* Harvest path: the same statistics without touching every row of every node (ss_nodes.hip).  match_node reads
 * <db>/kmers/<id> and looks every row up in the dump (identify.py:116-124) for each visited node; a sample has
 * hits in a few dozen of an E. coli database's 1645 nodes.
 *   ss_nodes_bind               once per (node set, database): (counter, list position) pairs sorted by counter
 *   ss_nodes_harvest_dev        after a scan: one streaming pass moves the non-zero counters to their list positions
 *                               in a node-major buffer and flags their nodes
 *   ss_nodes_reduce_touched_dev statistics of all nodes (untouched ones: length, zeros), buffer and flags cleared
 * Several GPUs, between the two (dist.py): touched flags MAX-all-reduced (get/set), the touched nodes' segments packed
 * (ss_nodes_pack_dev; packed_dev = NULL only returns the size; needs a host sync for that size), summed, unpacked.
 * The product path uses the CAPPED forms, which never wait for the host: the first `cap` packed counts go into the
 * buffer, the full packed size is left in *total_dev for the caller to read when it reads the statistics (total > cap:
 * harvest again and exchange with a larger cap; dist.exchange_touched keeps cap at about twice the last total).
 * ss_nodes_clear_dev zeroes the buffer and the flags (after a failed exchange, before the next harvest). */
int ss_nodes_bind(ss_nodes *ns, const ss_db *db);
int ss_nodes_harvest_dev(ss_nodes *ns, const ss_db *db, void *stream);
int ss_nodes_reduce_touched_dev(ss_nodes *ns, ss_node_stat *stats_dev, void *stream);
int ss_nodes_touched_get_dev(const ss_nodes *ns, uint32_t *flags_dev, void *stream);
int ss_nodes_touched_set_dev(ss_nodes *ns, const uint32_t *flags_dev, void *stream);
int ss_nodes_pack_dev(ss_nodes *ns, uint32_t *packed_dev, uint64_t cap, uint64_t *n_packed, void *stream);
int ss_nodes_unpack_dev(ss_nodes *ns, const uint32_t *packed_dev, void *stream);
int ss_nodes_pack_capped_dev(ss_nodes *ns, uint32_t *packed_dev, uint64_t cap, uint64_t *total_dev, void *stream);
int ss_nodes_unpack_capped_dev(ss_nodes *ns, const uint32_t *packed_dev, uint64_t cap, void *stream);
int ss_nodes_clear_dev(ss_nodes *ns, void *stream);
/* one ad-hoc row list (adjust_profile's `remain` set, identify.py:181-189) */
int ss_rows_reduce(const ss_db *db, const uint32_t *rows, uint64_t n, ss_node_stat *stat);

/* --------------------------------------------------------------------------------------------
 * Layer 2: the k-mer x strain matrix of one cluster as bit planes
 * (library/identify_strains_L2_Enet_Pscan_new_sp.py:191-201 densifies all_strains_re.npz into
 * int8; here one bit per entry, plane-major, K bits per strain padded to 128-bit words).
 * Bit vectors passed in (A, B, nu) are device arrays of words_per_plane dwords, bit k of row k
 * at word k/32, bit k%32.
 * ------------------------------------------------------------------------------------------ */
typedef struct ss_l2 ss_l2;
/* CSR of the K x S binary matrix (scipy.sparse.load_npz of all_strains_re.npz, :200) */
int ss_l2_create(const int64_t *indptr, const int32_t *indices, uint64_t K, uint32_t S, ss_l2 **out);
/* The same with the column indices already in DEVICE memory (4-byte aligned; read, not kept).  With ss_npz_member_dev: the
 * `indices.npy` member of all_strains_re.npz inflated on the device and packed from there -- a first run against a database
 * spent 2.3 of its 3.5 s inflating these members on one host thread (np.load), 2.5 GB for a 5 M x 300 cluster. */
int ss_l2_create_dev(const int64_t *indptr, const int32_t *indices_dev, uint64_t K, uint32_t S, ss_l2 **out);
/* A member of a ZIP archive (scipy.sparse.save_npz writes one .npy array per member: Recls_withR_new.py:110-112,
 * Build_overlap_matrix_sp.py:89-98) brought to the device: the member's data at [off, off + comp_n) of `path`, content CRC-32
 * and length as the archive's directory states them (both are checked).  method 8 (deflated): inflated on the device;
 * method 0 (stored): uploaded through pinned pieces whose CRCs are taken by the reading threads.  *d_data (64-byte aligned,
 * *n == usize bytes: the .npy header, then the array) is lent until ss_npz_member_done(*lease).  SS_ERANGE: the device
 * inflater declined (no dynamic-Huffman block to enter, an extreme ratio, too small) -- read the member on the host. */
int ss_npz_member_dev(const char *path, uint64_t off, uint64_t comp_n, uint32_t crc, uint64_t usize, int method, void **d_data,
                      uint64_t *n, void **lease);
int ss_npz_member_done(void *lease);
/* zlib's CRC-32 of (a prefix whose CRC-32 is prefix_crc) followed by n copies of `byte`, in O(log n): what the `data.npy`
 * member of a binary matrix must have for its content to be nnz ones -- known without inflating it. */
int ss_crc32_repeat(uint32_t prefix_crc, int byte, uint64_t n, uint32_t *out);
/* The same matrix as ready-made bit planes: planes[s * W + k / 32] bit k % 32, W = words_per_plane =
 * ((K + 31) / 32 rounded up to a multiple of 4), bits beyond K zero.  ss_l2_export_planes writes that
 * array (S * W dwords) from a handle: the host keeps it as a per-cluster image so that later runs skip
 * decompressing and re-packing all_strains_re.npz. */
int ss_l2_create_planes(const uint32_t *planes, uint64_t K, uint32_t S, ss_l2 **out);
/* A cluster image file of this package (the cache strainscan_amd writes beside SS_IMAGE_CACHE: bit planes + the overlap matrix's
 * CSR arrays at the given 64-byte-aligned offsets) straight to the device: planes AND overlap in one upload through pinned
 * buffers; equivalent to ss_l2_create_planes + ss_l2_set_overlap on the same arrays, same checks.  SS_EINVAL: not such a file.
 * (The handle's overlap arrays live inside that one allocation: ss_l2_set_overlap on an imported handle is SS_EINVAL.) */
int ss_l2_import(const char *path, uint64_t K, uint32_t S, uint64_t off_planes, uint64_t off_ptr, uint64_t off_idx, uint64_t off_val,
                 uint64_t nnz, uint32_t n_cols, ss_l2 **out);
int ss_l2_export_planes(const ss_l2 *h, uint32_t *planes);
int ss_l2_destroy(ss_l2 *h);
int ss_l2_info(const ss_l2 *h, uint64_t *K, uint32_t *S, uint64_t *words_per_plane);
/* The O(K) vector bookkeeping of detect_strains on the device (round 4; it was a dozen single-threaded numpy passes over
 * K rows: 83 ms of a 5 M-row cluster's solve).  ss_l2_set_overlap: overlap_matrix.npz as CSR (int8 K x n_cols), once per
 * cluster.  ss_l2_prepare (:191-197, 36-38, 402-415): y_host = input_y as int64[K]; col_sel[c] = how often column c is
 * among the identified clusters' columns (`overlap.A[:, all_cls - 1]`); writes y and y_u = y * ln as uint32[K], the bit
 * vectors [y > 1], [y_u > 1], [row kept: npp25 <= y <= min(npp75, npp_out)] (W words each) and y of the kept rows (0
 * elsewhere); out = {kept rows, any y_u > 0, a count negative or beyond 32 bits}.  ss_l2_fold: the fold words of
 * ss_l2_pattern_stats from the kept-row bit vector and ShuffleSplit's test bits per kept row (host, n_keep words).
 * ss_l2_count_keep: out[0] of ss_l2_prepare from y alone, on host threads (2 ms for 5 M rows): ShuffleSplit depends on the
 * number of kept rows only and is the longest step of a large cluster's solve -- it starts before y is on the device. */
int ss_l2_count_keep(const int64_t *y_host, uint64_t K, double npp25, double npp75, double npp_out, uint64_t *n_keep);
int ss_l2_set_overlap(ss_l2 *h, const int64_t *indptr, const int32_t *indices, const int8_t *data, uint32_t n_cols);
int ss_l2_prepare(const ss_l2 *h, const int64_t *y_host, const uint8_t *col_sel, double npp25, double npp75, double npp_out,
                  uint32_t *y_dev, uint32_t *yu_dev, uint32_t *G_dev, uint32_t *Gu_dev, uint32_t *keep_dev, uint32_t *ykeep_dev,
                  uint64_t out[3]);
int ss_l2_fold(const ss_l2 *h, const uint32_t *keep_dev, const uint32_t *split_bits, uint64_t n_keep, uint32_t *fold_dev);
/* ShuffleSplit(n_splits, test_size, random_state = seed) of scikit-learn (identify_strains_L2_Enet_Pscan_new_sp.py:433-442) with the
 * swaps on the device: the host walks the one sequential MT19937 word stream of the 20 permutations on a thread of its own and
 * hands each split's partners of the rows n - 1 .. n_test to the device, which finds every row's final element without
 * replaying the swap chain (ss_host.hip).  start returns at once; wait joins, synchronises and gives uint32[n] ON THE
 * DEVICE: bit f of entry e = row e is in the TRAINING half of split f (the test half is its complement).  1 <= n_test < n.
 * ss_l2_fold_train is ss_l2_fold with these bits (no host copy of the splits at all). */
typedef struct ss_split ss_split;
int ss_split_dev_start(uint64_t n, int n_splits, uint64_t n_test, uint32_t seed, ss_split **out);
int ss_split_dev_wait(ss_split *s, const uint32_t **train_bits_dev, double *walk_ms);
int ss_split_dev_free(ss_split *s);
int ss_l2_fold_train(const ss_l2 *h, const uint32_t *keep_dev, const uint32_t *train_bits_dev, uint64_t n_keep, int n_splits, uint32_t *fold_dev);
/* out1[s] = |X_s & A|, out2[s] = |X_s & A & B|; NULL = all ones.  Serves stat_cov/cal_cov_all
 * (:33-49: A = NULL, B = [y > 1]), get_remainc (:94-108) and get_candidate_arr (:121-134):
 * A = not-yet-used k-mers, B = [y_u > 1] or [y > 1]. */
int ss_l2_popc2(const ss_l2 *h, const uint32_t *A_dev, const uint32_t *B_dev, uint64_t *out1, uint64_t *out2);
/* nu &= ~X_col : "used_kmer = used_kmer + pXt[candidate]; used_kmer[used_kmer>1]=1" (:367-369) */
int ss_l2_andnot_col(const ss_l2 *h, uint32_t col, uint32_t *nu_dev);
/* For each listed column: over rows with X = 1 and y != 0, n_nz = how many, v_lo / v_hi =
 * np.percentile(.., q_lo / q_hi, interpolation='nearest'), cnt_in / sum_in = size and sum of the
 * values inside [v_lo, v_hi].  optimize_dominat_y (:136-175, q = 5/95, uses sum_in) and
 * get_avg_depth (:110-120, q = 25/75, uses sum_in / cnt_in). */
int ss_l2_quantile_sums(const ss_l2 *h, const uint32_t *y_dev, const uint32_t *cols, uint32_t ncols, double q_lo,
                        double q_hi, uint64_t *n_nz, uint32_t *v_lo, uint32_t *v_hi, uint64_t *cnt_in,
                        uint64_t *sum_in);
/* Sufficient statistics of the elastic net over the p <= 16 selected columns: for every p-bit row
 * pattern m, {rows, sum y, sum y^2} over (f < n_folds) the kept rows in the TEST half of fold f,
 * and (f = n_folds) all kept rows.  fold_dev[k]: bit 31 = row kept by the filter of :402-415,
 * bit f = row in the test half of ShuffleSplit fold f.  stats: host, [(n_folds+1)][2^p][3]. */
int ss_l2_pattern_stats(const ss_l2 *h, const uint32_t *cols, int p, const uint32_t *y_dev,
                        const uint32_t *fold_dev, int n_folds, uint64_t *stats);

/* --------------------------------------------------------------------------------------------
 * Positive elastic-net coordinate descent along a descending alpha path, warm-started, on Gram
 * statistics -- scikit-learn's _cd_fast.enet_coordinate_descent_gram inside enet_path
 * (ElasticNetCV at identify_strains...:437-442) and, with F = 1 and one alpha, the refit of
 * ElasticNet(...).fit (:451-455).  One workgroup per problem f < F.  All pointers are host
 * memory: Q [F][p][p], q [F][p], yy / n_train / n_test [F]; test_stats [F][2^p][3] (from
 * ss_l2_pattern_stats) or NULL; out: mse [n_alphas][F] (needs test_stats), coefs
 * [F][n_alphas][p], iters / gaps [F][n_alphas] (any may be NULL).
 * ------------------------------------------------------------------------------------------ */
int ss_enet_path_gram(const double *Q, const double *q, const double *yy, const double *n_train,
                      const double *n_test, int F, int p, const double *alphas, int n_alphas, double l1_ratio,
                      int max_iter, double tol, int positive, const uint64_t *test_stats, double *mse,
                      double *coefs, int *iters, double *gaps);

/* The same coordinate descent in its RESIDUAL form -- scikit-learn's _cd_fast.enet_coordinate_descent, what
 * ElasticNet(alpha, precompute=False).fit runs at identify_strains...:451-455 -- for callers that hold the design matrix
 * itself: R = y - X w lives on the device beside X, one pass over the rows per coordinate (32 B per row), block sums added
 * in a fixed order.  X: host, column-major [p][N] doubles (Fortran order, as scikit-learn holds it), p <= 64; y: host [N];
 * w [p]: in = the start, out = the coefficients; l1 = alpha * l1_ratio * N, l2 = alpha * (1 - l1_ratio) * N as
 * ElasticNet.fit passes them; gap / n_iter as the Cython routine returns them (may be NULL).  [The product's refit uses
 * ss_enet_path_gram with F = 1: for binary columns the Gram statistics are exact and p x p.] */
int ss_enet_cd(const double *X, const double *y, uint64_t N, int p, double l1, double l2, int max_iter, double tol,
               int positive, double *w, double *gap, int *n_iter);

#ifdef __cplusplus
}
#endif
#endif /* STRAINSCAN_HIP_H */
