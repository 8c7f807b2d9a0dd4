/* gwa.h -- C ABI of the MI355X-native genome-weaver `align` path (drop-in boundary).
 *
 * Replaces, for the single-end FM-index path, the reference's Java plugin surface:
 *   interface Aligner { void align(Read read, Reporter out) }      A/Aligner.java:30-33
 *   Align.query(...) strategy selection (-m bsf, -m sf)              A/Align.java:112-140
 *   Reporter.emit -> SAMOutput.emit -> AlignmentRecord.toSAMLine     J/parallel/Reporter.java:27-30,
 *                                                                    A/SAMOutput.java:73-82
 *   FMIndexOnGenome.load / buildFromSequence                         A/FMIndexOnGenome.java:60-115
 *   SequenceBoundary.toSAMHeader                                     A/SequenceBoundary.java:81-87
 * (paths relative to align/src/main/java/org/utgenome/weaver/; A = align/, J = .)
 *
 * Conventions: 0 = OK, negative = error (message via gwa_last_error, thread-local).  A read on
 * which the reference would throw fails the whole batch (the reference aborts the run,
 * S/BidirectionalSuffixFilter.java:264-267).  Results are in input order.  Calls on one index
 * handle are serialised (one HIP stream per handle, one handle per GPU).  Plain pointers and
 * sizes only; no C++ or torch types cross this boundary.
 */
#ifndef GWA_H
#define GWA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gwa_index gwa_index_t;
typedef struct gwa_batch gwa_batch_t;

/* AlignmentConfig + AlignmentScoreConfig (A/AlignmentConfig.java:40-72, A/AlignmentScoreConfig.java:37-77);
 * defaults from gwa_config_default: k 0.1, bsf, besthit, L 5, g 1, e 4, s 1, M 1, N 3, G 11, E 4, S 11, P 5, W 31,
 * sam_tags 0 */
typedef struct {
  float k;
  int32_t strategy;    /* 0 = bsf (-m bsf), 1 = sf (-m sf, S/SuffixFilter.java); others are rejected */
  int32_t report_type; /* 0 besthit, 1 allhits, 2 topL (-R) */
  int32_t top_l;       /* -L */
  int32_t num_gap_open, num_gap_ext, num_split; /* -g -e -s */
  int32_t match, mismatch, gap_open, gap_ext, split_open; /* -M -N -G -E -S */
  int32_t indel_end_skip, band_width; /* -P -W */
  uint32_t sam_tags;   /* optional SAM tags, GWA_SAM_TAG_* bits; 0 = the reference's lines.  A bit that is not
                        * defined fails gwa_batch_create*, gwa_align_* and gwa_pipeline_open
                        * ("gwa_config_t.sam_tags: unknown bits 0x..") */
} gwa_config_t;
/* MD:Z on every mapped line (FLAG without 0x4, RNAME a contig), appended last, after X0:i: "\tMD:Z:<value>".
 * Every path that formats SAM carries it: single and paired batches, results / results_range /
 * results_select, gwa_batch_format + gwa_batch_sam_copy and the gwa_pipeline_* calls.  Removing
 * "\tMD:Z:[^\t\n]*" from every line gives the default output byte for byte.
 * The reference prints no MD, and some of its lines are not SAM-spec alignments (POS <= 0, an S inside
 * the CIGAR, an alignment running past its contig's end), so the value is defined from the printed line
 * alone: walk the printed CIGAR from q = 0 in the printed SEQ and r = POS on the printed contig; M / X
 * compare SEQ[q] with the contig's base at r (a match iff both are one of A C G T and equal; a mismatch
 * prints the run of matches, then the contig's letter), D prints the run, '^' and the contig's letters,
 * N advances r, I and S advance q.  A position outside [1, contig length] reads as N (never a
 * neighbouring contig's base), as does SEQ past its end.  The value matches
 * [0-9]+(([ACGTN]|\^[ACGTN]+)[0-9]+)*; an empty CIGAR gives "0".  NM:i stays the reference's
 * numMismatches, which counts a read's N as A: NM and MD may disagree where the read has an N. */
#define GWA_SAM_TAG_MD 1u

/* A batch of reads, SoA, caller-owned.  Read i = name[name_off[i], name_off[i+1]), etc.
 * qual may be NULL: no read has a quality (SAM QUAL "*", as for FASTA input / -q queries).
 * qual_null (optional, may be NULL) marks single reads without one, one byte per read: nonzero =
 * read i's Read.getQual(0) is null (R/SingleEndRead.java:74-76, FASTA records) and its QUAL prints
 * "*" (R/AlignmentRecord.java:157) -- its qual_off range is ignored.  Zero-initialise the struct. */
typedef struct {
  uint32_t n;
  const char *name, *seq, *qual;
  const uint64_t *name_off, *seq_off, *qual_off;
  const uint8_t *qual_null;
} gwa_reads_t;

/* Reads parsed by the library from FASTA / FASTQ text (gwa_reads_parse); `reads` points into
 * library-owned blobs until gwa_reads_free.  Replaces the reference's read-file readers
 * (R/ReadReaderFactory.java:126-151, utgb FastqReader: unvendored, record rules in reads_io.cpp). */
typedef struct {
  gwa_reads_t reads;
  void *priv;
} gwa_read_buf_t;

/* One SAM record as the fields of the reference's AlignmentRecord (R/AlignmentRecord.java:44-79:
 * readName, chr, strand, start, end, numMismatches, cigar, querySeq, qual, score = 1, numBestHits,
 * alignmentState, split), so a JVM binding can build the objects SAMOutput.emit prints
 * (A/SAMOutput.java:73-82).  String fields are (offset, length) into gwa_results_t.sam. */
typedef struct {
  uint32_t read;          /* input index of the read */
  uint32_t flag;          /* SAM FLAG */
  int32_t ref;            /* contig index of chr; -1 = "*" */
  int32_t pos;            /* start */
  int32_t end;            /* end where the text fixes it (a split record: POS + TLEN of its first line), else pos */
  int32_t strand;         /* 0 = Strand.FORWARD, 1 = REVERSE (FLAG 0x10) */
  int32_t nm;             /* numMismatches: NM:i, -1 when the line has none */
  int32_t x0;             /* numBestHits: X0:i, 0 when absent (unmapped) */
  int32_t split;          /* index (in the record array) of this record's split record, -1 = none */
  int32_t is_split;       /* 1: this record is another record's split (emit the first one only) */
  int32_t qual_null;      /* 1: QUAL is "*" (qual == null) */
  int32_t pad_;
  uint64_t line_off, name_off, cigar_off, seq_off, qual_off, state_off;
  uint32_t line_len, name_len, cigar_len, seq_len, qual_len, state_len;
  uint64_t md_off;        /* the MD:Z value (GWA_SAM_TAG_MD); 0 / 0 when the line has none */
  uint32_t md_len;
  uint32_t pad2_;
} gwa_record_t;

/* Library-owned SAM text (no header), in input order; read i's lines are
 * sam[line_off[i], line_off[i+1]).  Free with gwa_results_free.  records / n_records are filled on
 * request by gwa_results_records (NULL / 0 until then).  paired = 1: results of a paired-end batch,
 * unit i = pair i, two mate lines (mate 1, mate 2), never split records. */
typedef struct {
  uint32_t n_reads;
  char *sam;
  uint64_t sam_len;
  uint64_t *line_off; /* n_reads + 1 */
  gwa_record_t *records;
  uint64_t n_records;
  uint32_t paired;
} gwa_results_t;

/* Per-batch counters (instrumentation for SURVEY.md §8d roofline accounting). */
typedef struct {
  double kernel_ms;        /* device time of all kernels of gwa_batch_run: encode + align (HIP events) */
  double quickscan_ms;     /* fm_quickscan kernel */
  double search_ms;        /* bsf_search kernels (all tiers) */
  uint64_t fm_searches;    /* numFMIndexSearches summed over reads */
  uint64_t quick_steps;    /* FMQuickScan steps */
  uint64_t blocks;         /* 64-B Occ blocks read (algorithmic bytes = 64 * blocks) */
  uint64_t quick_blocks;   /* of which by fm_quickscan */
  uint64_t states;         /* search states created */
  uint64_t sa_reads;       /* 4-B suffix-array gathers (exact hits + verifications) */
  uint32_t tier_reads[4];  /* reads processed per capacity tier */
  uint32_t n_mapped, n_unmapped;
  uint64_t kmer_lookups;   /* 8-B k-mer interval-table reads by fm_quickscan */
  uint64_t quick_short_steps; /* FMQuickScan steps answered without Occ blocks (k-mer table, single-row text compare) */
  uint64_t quick_sa_reads; /* of sa_reads, by fm_quickscan */
  uint64_t search_short_steps; /* search FM steps answered by one text character (single-row states) */
  float tier_ms[4];        /* search time per capacity tier (HIP events) */
  uint64_t num_sw;         /* DP verifications (alignBlockDetailed calls) */
  uint64_t verify_bytes;   /* SURVEY.md 8(d) bytes of those verifications (reference window + Peq) */
  uint64_t quick_text_runs; /* fm_quickscan text-mode runs (one 32-base 2-bit text window + N flags each) */
  double encode_ms;        /* read encoding on the device at the start of gwa_batch_run (part of kernel_ms) */
  double format_ms;        /* the last SAM formatting of the batch on the device (gwa_batch_format / results) */
  double rescue_ms;        /* paired-end batches: pair choice + mate rescue kernels (part of kernel_ms) */
  uint64_t heavy_pairs;    /* paired-end batches: pairs chosen by the sorted sweep (> 64 candidate combinations) */
  uint64_t rescue_window_skipped; /* paired-end: mate rescues not tried, because the mate is longer than
                                   * 256 bp or the window the insert range allows (max_insert - min_insert
                                   * + m + 2 kr) exceeds 320 bases */
  double compress_ms;      /* the last BGZF compression of the batch's SAM text on the device: block kernel,
                            * size scan and compaction (gwa_batch_format_bgzf / results_bgzf; HIP events) */
  uint64_t bgzf_bytes;     /* its output, */
  uint64_t bgzf_blocks;    /* blocks (ceil(SAM bytes / 65280)) */
  uint64_t bgzf_stored;    /* and how many of them are stored blocks (deflate would not have been smaller) */
  double bam_ms;           /* the last BAM record formatting of the batch on the device (gwa_batch_format_bam /
                            * results_bam_records / results_bam; HIP events).  compress_ms and the bgzf_* fields
                            * describe the last compression, of SAM text or of BAM records */
  uint64_t bam_bytes;      /* its output: the uncompressed records */
} gwa_batch_stats_t;

void gwa_config_default(gwa_config_t *cfg);
const char *gwa_last_error(void);
int gwa_device_count(void);

/* Build an index from FASTA text (the `bwt` command: PackFasta + cyclic SA + BWT) and place
 * it in HBM of `device`. */
int gwa_index_build_fasta(const char *fasta_text, uint64_t len, int device, gwa_index_t **out);
/* Same, from a file (the `-r` argument): a FASTA file, or an index saved by gwa_index_save (recognised
 * by its magic), which skips the FASTA parse. */
int gwa_index_open(const char *fasta_path, int device, gwa_index_t **out);
/* Save an index (2-bit text, N bitmap, contig table; the suffix arrays and Occ blocks are rebuilt on
 * the GPU at load).  Plays the role of the reference's `bwt` command output (A/BWTransform.java:72-179,
 * A/BWTFiles.java:40-80) in this build's own format. */
int gwa_index_save(const gwa_index_t *ix, const char *path);
/* Same, from codes 0..4 (A,C,G,T,N) and a contig table (names + lengths, concatenated in order). */
int gwa_index_build_codes(const uint8_t *codes, uint64_t n, int32_t n_contigs, const char *const *names,
                          const int64_t *lengths, int device, gwa_index_t **out);
uint64_t gwa_index_text_size(const gwa_index_t *ix);
uint64_t gwa_index_device_bytes(const gwa_index_t *ix);
/* Export the cyclic suffix array of strand 0 (text) or 1 (reversed text), n entries. */
int gwa_index_export_sa(const gwa_index_t *ix, int strand, uint32_t *out);
int gwa_sam_header(const gwa_index_t *ix, char **text, uint64_t *len);
void gwa_index_close(gwa_index_t *ix);

/* One call per batch: H2D, align on the GPU, D2H, SAM formatting. */
int gwa_align_batch(gwa_index_t *ix, const gwa_config_t *cfg, const gwa_reads_t *reads, gwa_results_t *out);
void gwa_results_free(gwa_results_t *r);
/* Fill r->records (one gwa_record_t per SAM line, in text order) from the SAM text of r. */
int gwa_results_records(const gwa_index_t *ix, gwa_results_t *r);
void gwa_free(void *p);

/* Parse the complete records of text[0, len): format 0 = FASTA, 1 = FASTQ.  With final = 0 the
 * last record may continue past len and is left for the next call; *consumed = bytes parsed
 * (the caller keeps text[*consumed, len) in front of its next chunk).  <0 on a malformed record. */
int gwa_reads_parse(const char *text, uint64_t len, int format, int final, gwa_read_buf_t *out, uint64_t *consumed);
void gwa_reads_free(gwa_read_buf_t *b);

/* Split form used by bench.py: upload once (reads resident in HBM), run the kernels (timed),
 * then fetch results. */
int gwa_batch_create(gwa_index_t *ix, const gwa_config_t *cfg, const gwa_reads_t *reads, gwa_batch_t **out);
int gwa_batch_run(gwa_batch_t *b);
/* Paired-end batch (config C5; the build's own design -- the reference has no paired-end path,
 * R/ReadReaderFactory.java:60-84): mate1[i] and mate2[i] form pair i.  Each mate is aligned as a
 * single-end read (-m bsf, every best hit kept); the pair of hits on one contig, opposite strands,
 * forward-reverse, with template length in [min_insert, max_insert] and the fewest differences wins
 * (rules: oracle/gwa_oracle.cpp orc_align_pairs).  Results hold two SAM lines per pair (n_reads =
 * pairs, line_off per pair) with mate fields and TLEN.
 * Mate rescue (rule 3) aligns the other mate inside the window the insert range allows next to the
 * anchor; it is tried for mates of at most 256 bp and windows of at most 320 bases (max_insert -
 * min_insert + m + 2 max(k, m / 10); the default 210-390 gives 300 for 100 bp mates).  Longer mates
 * and wider windows skip the rescue and are counted in gwa_batch_stats_t.rescue_window_skipped. */
int gwa_batch_create_pairs(gwa_index_t *ix, const gwa_config_t *cfg, const gwa_reads_t *mate1, const gwa_reads_t *mate2,
                           int32_t min_insert, int32_t max_insert, gwa_batch_t **out);
/* One call per paired batch: create_pairs + run + results. */
int gwa_align_pairs(gwa_index_t *ix, const gwa_config_t *cfg, const gwa_reads_t *mate1, const gwa_reads_t *mate2,
                    int32_t min_insert, int32_t max_insert, gwa_results_t *out);
int gwa_batch_stats(gwa_batch_t *b, gwa_batch_stats_t *st);
int gwa_batch_results(gwa_batch_t *b, gwa_results_t *out);
/* The batch's SAM text written in HBM only (paired-end: pairing included); *sam_bytes = its size.
 * For timing the device side of the reporting path; gwa_batch_results copies the text out. */
int gwa_batch_format(gwa_batch_t *b, uint64_t *sam_bytes);
/* Device-to-device copy of the batch's SAM text as the last gwa_batch_format wrote it in HBM (input
 * order, no header) into dst, device memory of the batch's GPU with room for *len bytes; with dst NULL
 * only *len is set.  Fails unless the last formatting of the batch was gwa_batch_format.  For a
 * device-side gather of the SAM of several GPUs over RCCL / xGMI (genome-weaver-align_amd/dist.py
 * gather_sam_device; SURVEY.md §8e's optional collective). */
int gwa_batch_sam_copy(gwa_batch_t *b, void *dst, uint64_t *len);

/* ---- BGZF output (the blocked gzip of the SAM specification, section 4.1), compressed on the device ----
 * The compressed form of a text T is one BGZF block per 65 280-byte slice of T (the last slice shorter;
 * an empty T gives no block).  A block is the 18 header bytes 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43
 * 02 00 + BSIZE (u16 LE, block size - 1), one raw deflate stream that is a single final block with
 * dynamic Huffman codes (match lengths 3-258, distances 1-32768, never reaching before the slice), then
 * CRC32 and ISIZE (u32 LE each) of the slice.  Where the deflate payload would exceed the slice's length
 * + 5 bytes the block is a stored block, so every block is at most 65 311 bytes.  The blocks in order
 * decompress to T byte for byte (gzip -d, zcat, htslib), and the same T gives the same bytes on every
 * run, on the device and in the host build of the encoder.  The reference has no compressed output. */
#define GWA_OUT_SAM  0u
#define GWA_OUT_BGZF 1u
/* The batch's SAM text formatted and compressed in HBM only (timing counterpart of gwa_batch_format, which
 * it includes: gwa_batch_sam_copy gives the plain text afterwards). */
int gwa_batch_format_bgzf(gwa_batch_t *b, uint64_t *bgzf_bytes, uint64_t *n_blocks);
/* The same bytes in library-owned host memory (gwa_free).  -m bd / -m bwa: no block. */
int gwa_batch_results_bgzf(gwa_batch_t *b, uint8_t **out, uint64_t *len);
/* Any bytes -> BGZF blocks (no EOF marker) in library-owned memory (gwa_free): device >= 0 runs the
 * kernels there, device < 0 the host build of the same encoder (no GPU needed); identical bytes. */
int gwa_bgzf_compress(int device, const void *in, uint64_t n, uint8_t **out, uint64_t *out_len);
/* The 28-byte end-of-file marker of the specification (an empty block). */
int gwa_bgzf_eof(uint8_t *out28);
/* ---- BGZF input: the same container inflated on the device ----
 * The input is any concatenation of BGZF members (what gwa_bgzf_compress, bgzip and htslib write): a gzip
 * member with CM 8 and FLG = FEXTRA whose extra field holds a BC subfield of length 2 (other subfields may
 * stand before or after it) with BSIZE = the member's size - 1, a raw deflate payload, CRC32 and ISIZE <=
 * 65 536.  Empty members -- the 28-byte EOF marker among them -- may stand anywhere.  The payload may be any
 * deflate stream: any number of stored, fixed and dynamic blocks, codes of up to 15 bits, lengths 3-258,
 * distances 1-32 768 that never reach before the member's own output.  The headers are walked on the host;
 * each payload is inflated by one workgroup (device >= 0) or by the host build of the same decoder (device
 * < 0, no GPU needed), which also checks that exactly ISIZE bytes come out and that their CRC32 is the
 * trailer's.  Both give identical bytes and identical errors.  No access of the decoder depends on the
 * payload being well formed: a malformed member ends the call with a negative status and gwa_last_error()
 * = "BGZF member <index> at byte <offset in the input>: <what was wrong>"; for a payload the decoder refused,
 * <what> ends in "at payload bit <offset> (status <code>)" with the codes 1 reserved block type, 2 stored
 * LEN/NLEN mismatch, 3 payload ends inside a block, 4 HLIT > 286 or HDIST > 30, 5 invalid code-length code,
 * 6 bad code-length repeat, 7 no end-of-block code, 8 over-subscribed or incomplete code set, 9 invalid code
 * or symbol, 10 distance before the member's output, 11 length differs from ISIZE, 12 CRC32 mismatch.
 * The result is library-owned (gwa_free).  The reference reads .gz input with java.util.zip on one thread. */
int gwa_bgzf_decompress(int device, const uint8_t *in, uint64_t n, uint8_t **out, uint64_t *out_len);
/* For timing the kernel alone: the same with the compressed bytes resident in HBM and the kernel launched
 * `repeat` times; *kernel_ms = the last launch between HIP events.  The text is discarded. */
int gwa_bgzf_decompress_timed(int device, const uint8_t *in, uint64_t n, int repeat, uint64_t *out_len, double *kernel_ms);
/* ---- BAM output: alignment records built on the device, in the BGZF container above ----
 * The reference has no BAM, and some lines it prints are not SAM-spec alignments, so a record is a total
 * function of the printed SAM line (with the batch's sam_tags), as MD is.  Layout: the BAMv1 alignment record
 * of the SAM specification section 4.2, little-endian: block_size, refID, pos, l_read_name (u8), mapq (u8),
 * bin (u16), n_cigar_op (u16), flag (u16), l_seq (u32), next_refID, next_pos, tlen, read_name NUL, cigar, seq,
 * qual, tags.
 *   refID       index of the contig RNAME names; -1 for "*", the empty name and a line without a contig
 *   next_refID  the same of RNEXT; "=" gives this line's refID; "*" gives -1 and next_pos -1
 *   pos, next_pos  POS - 1 and PNEXT - 1 as they are (POS 0 gives -1, a negative POS keeps its two's complement)
 *   tlen        TLEN (its low 32 bits);  mapq 1, the column the reference always prints;  flag FLAG
 *   read_name   the QNAME bytes and a NUL (an empty name: the NUL alone).  A name longer than 254 bytes fails
 *               the batch: "BAM: read <index> has a name of <n> bytes (at most 254 fit a record)"
 *   cigar       the printed elements, len << 4 | op with op from MIDNSHP=X (the writer prints no '=');
 *               an empty CIGAR and "*" give n_cigar_op 0
 *   seq         SEQ at 4 bits per base, A 1, C 2, G 4, T 8, N 15, the first base of a byte in its high nibble,
 *               the unused low nibble of an odd l_seq 0; an empty SEQ gives l_seq 0
 *   qual        l_seq bytes: the QUAL bytes - 33 (mod 256) where QUAL has exactly l_seq bytes (a "*" next to a
 *               one-base SEQ is such a byte), otherwise 0xFF each (QUAL "*", and a split record whose quality
 *               substring and SEQ differ in length)
 *   bin         4680 (reg2bin(-1, 0)) for FLAG 0x4 or pos < 0, else the specification's reg2bin(pos, pos +
 *               max(reflen, 1)), reflen = the sum of the M, D, N and X elements
 *   tags        those printed, in the printed order: NM as int32 (type i), XP as Z, X0 as int32 (type i), MD as
 *               Z (GWA_SAM_TAG_MD, the text's value); the integer types are fixed, so a record's size does not
 *               depend on a tag's value
 * Where the SAM writer fails (the reference would throw), the BAM writer fails the same way.  The same batch
 * gives the same bytes on every run, from the device and from the host build (csrc/bam_core.h).
 * A BAM file is BGZF(gwa_bam_header) + BGZF(records of batch 0) + BGZF(records of batch 1) ... + the EOF
 * marker; every part is its own run of blocks (a short block at its end), and records may straddle the
 * 65 280-byte slices inside a part. */
#define GWA_OUT_BAM 2u
/* The batch's BAM records written in HBM only (timing counterpart of gwa_batch_format); *bam_bytes = their
 * size.  gwa_batch_sam_copy fails afterwards: the last formatting was not gwa_batch_format's. */
int gwa_batch_format_bam(gwa_batch_t *b, uint64_t *bam_bytes);
/* The uncompressed records in library-owned host memory (gwa_free).  -m bd / -m bwa: no record. */
int gwa_batch_results_bam_records(gwa_batch_t *b, uint8_t **out, uint64_t *len);
/* The same bytes as BGZF blocks (no EOF marker), compressed on the device. */
int gwa_batch_results_bam(gwa_batch_t *b, uint8_t **out, uint64_t *len);
/* The uncompressed BAM header (gwa_free), built on the host: "BAM\1", l_text and the text gwa_sam_header
 * returns, n_ref, and per contig l_name (with its NUL), the name as RNAME prints it, NUL, l_ref. */
int gwa_bam_header(const gwa_index_t *ix, uint8_t **out, uint64_t *len);
/* ---- BAM input: alignment records read as reads, decoded on the device ----
 * The reference reads no BAM.  A record is the BAMv1 alignment record laid out under "BAM output" above; what
 * the aligner takes from it is a read:
 *   name      the read_name bytes before the first NUL, as they are (no whitespace tokenising).  l_read_name 0,
 *             or no NUL inside l_read_name bytes, is an error.
 *   sequence  l_seq letters "=ACMGRSVTWYHKDBN"[nibble], the high nibble first.  With FLAG 0x10 the read is the
 *             reverse complement of the stored SEQ: A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; S, W, N and '='
 *             stay.  A letter other than A C G T is treated as that letter is in FASTQ text.
 *   quality   l_seq > 0 and qual[0] = 0xFF: the read has none (qual_null, QUAL "*"; the other bytes are not
 *             looked at).  l_seq = 0: the empty string, present, whatever byte follows.  Otherwise byte + 33 per
 *             base, reversed with FLAG 0x10; a byte above 93 is an error (it would not print as SAM QUAL).
 *   The input's CIGAR, tags, refID, pos, mapq and mate fields are ignored.  A record with FLAG 0x100 or 0x800
 *   (secondary, supplementary) is not a read: it is skipped and counts in no read index.
 * A file is BGZF members whose inflated bytes are "BAM\1", l_text, the text, n_ref, per contig l_name, name and
 * l_ref, then records to the end.  The header's contigs are ignored (the reference is the index).  Errors: a
 * wrong magic, a header cut off by the file's end -- both name the file -- and for records "BAM record <index>
 * at byte <offset in the inflated stream>: <what>", index counting all records, skipped ones too: a block_size
 * below 32 or below 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq (worded as
 * gwa_bam_sorter_add_records words it), a record reaching past the data, a chain that ends inside a
 * block_size field, and the name and quality errors above (the lowest such record).
 * Equivalence: aligning a BAM file gives, byte for byte, the output of aligning the same reads, in order,
 * handed over in memory as gwa_reads_t, qual_null set where a record has no quality; where every record has a
 * quality and l_seq >= 1, that is the output for the equivalent FASTQ file -- SAM, MD, BGZF, BAM, sorted BAM,
 * single and paired.
 * On the device: the host walks the block_size chain only; a length pass (one lane per record), a scan and
 * an unpack pass (16 lanes per record, 16 letters or quality characters per lane and step) produce the read
 * text in HBM; the names stay in the record bytes (csrc/bam_in.hip).
 *
 * Headerless records -> reads (free with gwa_reads_free; every read has a qual_off range, empty where qual_null
 * marks it).  The chain is validated first.  device >= 0 runs the kernels, device < 0 the host build of the same
 * decoder (no GPU needed); blobs, offsets, qual_null and errors are identical. */
int gwa_bam_reads_decode(int device, const uint8_t *records, uint64_t len, gwa_read_buf_t *out);
/* For timing the kernels alone: the records resident in HBM, length pass + scan + unpack launched `repeat`
 * times; *kernel_ms = the last round between HIP events, *n_reads = the reads. */
int gwa_bam_reads_decode_timed(int device, const uint8_t *records, uint64_t len, int repeat, uint64_t *n_reads,
                               double *kernel_ms);
/* Where the records start in an inflated BAM (bam[0, len) must hold the whole header).  Negative on a wrong
 * magic or an incomplete header. */
int gwa_bam_header_size(const uint8_t *bam, uint64_t len, uint64_t *header_bytes);
/* ---- Sorted BAM: the records in coordinate order, sorted on the device, and the .bai index ----
 * The reference has nothing here; every part of the rule is a function of the record bytes alone.
 * Order.  A record with refID >= 0 has key = (uint64)(uint32)refID << 32 | ((uint32)pos ^ 0x80000000): the
 *   signed pos orders, pos -1 and below come first on their contig.  refID -1 has key 0xFFFFFFFF00000000
 *   whatever its pos: such records go last.  The sorted stream is the input-order record stream stably sorted
 *   by key: equal keys keep input order (batch order, then the order of gwa_batch_results_bam_records, so
 *   mate 1 stays before mate 2).  The stream therefore does not depend on the batch size, the workers, the
 *   devices, the memory limit or spilling.
 * File.  BGZF(gwa_bam_header_sorted) + BGZF(sorted stream) + the EOF marker.  The header is gwa_bam_header's
 *   with the line "@HD\tVN:1.6\tSO:coordinate\n" before the @SQ text.  The whole sorted stream is one text T
 *   under the BGZF contract above (one block per 65 280-byte slice, the last one shorter), whatever parts the
 *   writer works in.  The same records give the same file for every batch size and memory limit, from the
 *   device and from the host build.
 * Index (.bai, SAM specification section 5.2, little-endian): "BAI\1", n_ref, per contig its bins and its
 *   linear index, then n_no_coor (u64).  The virtual offset of stream byte u is (H + the sizes of the blocks
 *   before block u / 65280) << 16 | u % 65280, H = where the stream starts in the file; a record's end offset
 *   is that at u + its size (on a slice edge: the next block, offset 0).  Indexed are the records with refID
 *   >= 0: beg = max(pos, 0), end = min(max(pos + max(reflen, 1), beg + 1), 2^29) with reflen the sum of the
 *   M, D, N, = and X elements, index bin = reg2bin(beg, end) (not the record's bin field).  Walking a contig's
 *   records in stream order, every maximal run of consecutive records with one index bin is one chunk [first
 *   record's offset, last record's end offset]; a bin's chunks stay in stream order and are not merged; bins
 *   ascend.  Pseudo-bin 37450 is the last bin of every contig that has a record (counted in n_bin, n_chunk 2:
 *   (first record's offset, last record's end offset), (n_mapped, n_unmapped) by FLAG 0x4).  A contig without
 *   records has n_bin 0 and n_intv 0.  Linear index: n_intv = ((largest end - 1) >> 14) + 1, ioffset[w] = the
 *   smallest offset of a record with beg >> 14 <= w <= (end - 1) >> 14, a window without one takes the next
 *   later window's.  n_no_coor counts the refID -1 records.  A contig longer than 2^29 fails index creation
 *   (the message names the contig, its length and the limit); sorting without an index still works.  No .csi. */
int gwa_bam_header_sorted(const gwa_index_t *ix, uint8_t **out, uint64_t *len);
/* The batch's BAM records formatted and sorted in HBM only (timing counterpart of gwa_batch_format_bam, which
 * it includes).  Passes: a walk over each unit's block_size chain (count, scan, keys and index fields), a
 * stable radix sort of (key, ordinal), a scan of the permuted sizes, and the gather of the records. */
int gwa_batch_format_bam_sorted(gwa_batch_t *b, uint64_t *bytes, uint64_t *n_records);
/* The sorted records and their keys (one per record, ascending) in library-owned host memory (gwa_free each). */
int gwa_batch_results_bam_sorted(gwa_batch_t *b, uint8_t **records, uint64_t *len, uint64_t **keys, uint64_t *n_records);
/* Device times of the batch's last sort (HIP events), its records and bytes. */
typedef struct {
  float walk_ms, sort_ms, permute_ms, gather_ms; /* walk + keys (on a batch's first sort also the allocation of
                                                  * its buffers); radix sort; permuted sizes and their scan (with the
                                                  * readback of the total); the gather kernel alone */
  uint64_t records, bytes;
} gwa_bam_sort_times_t;
int gwa_batch_bam_sort_times(gwa_batch_t *b, gwa_bam_sort_times_t *t);
/* The run sorter: one sorted run per batch, merged at finish.  A run is one batch's sorted records plus a
 * per-record array of 24 bytes per record (key, size, beg, end, index bin), which always stays in host memory.
 * run_id is the batch's number in input order; runs may be added in any order from any thread, and the result
 * depends on the ids only.  Record bytes stay in host memory up to mem_bytes in all; beyond that a run's bytes
 * go to a file of its own in tmp_dir (read back sequentially, unlinked at finish, close or failure); with
 * tmp_dir NULL such an add fails, naming both numbers.  device >= 0 sorts and compresses there, device < 0 runs
 * the host build of the same logic; identical bytes. */
typedef struct gwa_bam_sorter gwa_bam_sorter_t;
typedef struct {
  uint64_t records, bytes, runs, spilled_runs, spilled_bytes, blocks, out_bytes, bai_bytes;
  double add_s, order_s, copy_s, compress_s, write_s, index_s; /* add_s: summed over the adding threads, for
                                                                * add_batch with the batch's formatting, sort and copy to
                                                                * the host; the others: the stages of finish */
} gwa_bam_sorter_stats_t;
int gwa_bam_sorter_open(const gwa_index_t *ix, int device, const char *tmp_dir, uint64_t mem_bytes, gwa_bam_sorter_t **out);
/* The batch's records, formatted and sorted on the batch's device, as run run_id. */
int gwa_bam_sorter_add_batch(gwa_bam_sorter_t *s, uint64_t run_id, gwa_batch_t *b);
/* Unsorted caller records as run run_id.  The block_size chain is validated on the host first: every
 * block_size >= 32, name, CIGAR, SEQ and QUAL inside their record, the chain ending exactly at len; otherwise
 * "BAM record <index> at byte <offset>: <what>". */
int gwa_bam_sorter_add_records(gwa_bam_sorter_t *s, uint64_t run_id, const uint8_t *bytes, uint64_t len);
/* Orders all records (a stable sort of the concatenated keys with run-major ordinals), copies them run by
 * run, front to back, into parts of whole 65 280-byte slices, compresses each part and writes the blocks to
 * fd_bam; then builds the index on the host and writes it to fd_bai (-1: none).  Writes neither the header nor
 * the EOF marker; the stream's start in the file is lseek(fd_bam, 0, SEEK_CUR), so an index with a
 * non-seekable fd_bam is refused.  No run: no block, and an index of empty contigs.  The runs are consumed. */
int gwa_bam_sorter_finish(gwa_bam_sorter_t *s, int fd_bam, int fd_bai, gwa_bam_sorter_stats_t *stats);
void gwa_bam_sorter_close(gwa_bam_sorter_t *s);
/* ---- Duplicate marking: FLAG 0x400 set in the sorted file, decided on the device ----
 * Off by default; with it off every byte stays as above.  The reference has nothing here.  The rule is a
 * function of the input-order record stream alone: run ids ascending, inside a run the order in which the
 * records were handed over.
 * Participating record.  FLAG & (0x4 | 0x100 | 0x800) == 0 and refID >= 0.  Every other record is never marked
 *   and never influences a decision.
 * End key of a participating record.  u5 is the unclipped 5' coordinate, in int64: forward (FLAG & 0x10 == 0)
 *   pos - (the sum of the leading S and H elements); reverse pos + reflen + (the sum of the trailing S and H
 *   elements) - 1, reflen summed over M, D, N, = and X (no max(., 1)).  Leading and trailing: the maximal run of
 *   S/H elements at that end of the CIGAR; n_cigar_op == 0 gives u5 = pos on either strand.
 *   endKey = (uint64)(uint32)refID << 33 | (uint64)(uint32)((uint32)u5 + 0x80000000) << 1 | strand (u5 mod 2^32).
 * Templates.  Records i and i + 1 of one run's input order are a pair when both have FLAG 0x1, neither has
 *   0x100 or 0x800, i has 0x40 and not 0x80, i + 1 has 0x80 and not 0x40, and their l_read_name and name bytes
 *   are equal.  Every record not in a pair is a template of its own.  A pair never spans two runs: the batch
 *   writer never splits a unit, and a caller of gwa_bam_sorter_add_records who cuts a pair across two runs gets
 *   two single-record templates.  The two pieces of a split single-end read print as 0x1|0x40 and 0x1|0x80
 *   and are therefore a pair: intended.
 * Classes.  A pair with both records participating is a pair template, its signature (lo, hi): the two end
 *   keys ascending.  A template with exactly one participating record (an unpaired record, or a pair with one
 *   participating record) is a fragment template, its signature that record's endKey.  A template without a
 *   participating record is in neither class.
 * Score.  The sum over the template's participating records of the quality bytes q with 15 <= q <= 93 (a
 *   0xFF byte counts 0), held in a uint32.
 * Ordinal.  (run_id, input ordinal of the template's first record in the run), compared lexicographically: the
 *   global input order, whatever the batch size.
 * Decision.  Among pair templates with equal (lo, hi) the one with the highest score is kept, a tie goes to
 *   the lowest ordinal; the others are duplicates.  Among fragment templates with equal endKey: if any
 *   participating record of any pair template has that endKey, all of them are duplicates; otherwise the
 *   highest score is kept, ties to the lowest ordinal, the others are duplicates.  A duplicate template gets
 *   FLAG |= 0x400 on each of its participating records and on nothing else; no other byte of any record
 *   changes.  No optical duplicates, no libraries or read groups, no removal of records.
 * File.  As "Sorted BAM": order, slices and blocks unchanged (the flag is not part of the key), the .bai of the
 *   same structure (only its virtual offsets may move, as the blocks' sizes change with the bytes).  File and
 *   index depend on the record stream only: not on the batch size, the workers, the devices, the memory limit,
 *   spilling, or the device against the host build. */
/* Marking for the runs added from now on; fails once a run has been added (until the next finish). */
int gwa_bam_sorter_set_markdup(gwa_bam_sorter_t *s, int on);
typedef struct {
  uint64_t templates, pair_templates, frag_templates, dup_pair_templates, dup_frag_templates, dup_records;
  double keys_s, resolve_s; /* keys_s: the per-run passes (device: between HIP events), summed over the adds;
                             * resolve_s: the global resolve inside finish, with its copies */
} gwa_markdup_stats_t;
/* Of the last finish (all zero when marking was off). */
int gwa_bam_sorter_markdup_stats(const gwa_bam_sorter_t *s, gwa_markdup_stats_t *st);
/* Per record of gwa_batch_results_bam_sorted, in the same order, 24 bytes: endKey (u64; all ones: the record
 * does not participate), mateKey (u64; the other record's endKey in a pair template with both participating,
 * else all ones), score (u32, the template's), leader (u32, the batch-input ordinal of the template's first
 * record).  Library-owned host memory (gwa_free). */
int gwa_batch_results_bam_dupinfo(gwa_batch_t *b, uint8_t **info, uint64_t *n_records);
/* The same entries for caller records (validated as gwa_bam_sorter_add_records does), in input order, leader =
 * the input ordinal: the per-run pass on `device`, or its host build for device < 0; identical bytes. */
int gwa_bam_records_dupinfo(int device, const uint8_t *records, uint64_t len, uint8_t **info, uint64_t *n_records);
/* For timing the per-run kernel alone: the records (a valid block_size chain) resident in HBM, the kernel
 * launched `repeat` times; *kernel_ms = the last launch between HIP events, *n = the records. */
int gwa_bam_markdup_timed(int device, const uint8_t *records, uint64_t len, int repeat, uint64_t *n, double *kernel_ms);
/* SAM for reads [first, first+count) only (n_reads = count). */
int gwa_batch_results_range(gwa_batch_t *b, uint32_t first, uint32_t count, gwa_results_t *out);
void gwa_batch_free(gwa_batch_t *b);
/* SAM for the reads idx[0..count) in that order (n_reads = count). */
int gwa_batch_results_select(gwa_batch_t *b, const uint32_t *idx, uint32_t count, gwa_results_t *out);
/* Instrumentation: per-read counters after gwa_batch_run, GWA_READ_COUNTERS int32 per read:
 * [0] status, [1] fm_searches (numFMIndexSearches), [2] quick_steps (FMQuickScan steps),
 * [3] quickscan Occ blocks, [4] search Occ blocks, [5] search states, [6] SA gathers, [7] hits,
 * [8..11] quick-scan mismatches / longest-match start (forward, reverse; searched reads only),
 * [12] deepest search tier (-1 = finished in the quick scan), [13] k-mer table lookups,
 * [14] quick-scan steps answered without Occ blocks, [15] search steps answered from the text,
 * [16] DP verifications (numSW), [17] SURVEY.md 8(d) verify bytes, [18..19] 0. */
#define GWA_READ_COUNTERS 20
int gwa_batch_read_counters(gwa_batch_t *b, int32_t *out);

/* ---- Multi-device driver and overlapped host pipeline (8(f) row 2) ----
 * Replaces the reference's single-threaded read loop (A/Align.java:174-196: ReadReaderFactory ->
 * PassReadToAligner -> Aligner.align -> SAMOutput.emit, one read at a time).  A pipeline holds n_ix
 * index handles -- one per GPU, each a full replica -- and deals read batches of batch_reads reads
 * to them as they become free (workers_per_device host threads per handle overlap one batch's set-up
 * and SAM formatting with another's kernels).  Output is in input order, byte-identical to a
 * single-handle run.  The handles must outlive the pipeline.  workers_per_device <= 0 means 3.
 * The first gwa_pipeline_align_file call pins the read-text buffers a file run keeps in flight (sized
 * from the file, at most a quarter of the host's available memory; about 5.4 GB for a large file on
 * one device); they and each worker's pinned SAM buffer are kept for later calls.  In-memory runs
 * (gwa_pipeline_align) pin nothing.  Output to an O_APPEND descriptor or a pipe is written in batch
 * order with write(); to a regular file, each batch at its offset with pwrite(). */
typedef struct gwa_pipeline gwa_pipeline_t;
typedef struct {
  uint64_t reads, batches;
  double wall_s;               /* the last align / align_file call */
  double read_s;               /* of which reading (and decompressing) the read file */
  double device_kernel_s[16];  /* per handle: time inside gwa_batch_run */
  /* align_file stage times, summed over worker threads: read parse, batch set-up (H2D + encode),
   * SAM formatting + D2H, output writes, and waiting for the batch-order output position */
  double parse_s, setup_s, format_s, write_s, order_wait_s;
  double frame_s;  /* reader thread: framing the text into batches of complete records */
  uint64_t pinned_bufs;  /* align_file: pinned read-text buffers large enough for this file's chunks */
  uint64_t out_bytes;    /* align_file / align_pair_files: bytes written to fd (SAM text, or BGZF blocks) */
  /* BGZF read files (a .gz file whose first member has the BC subfield; GWA_BGZF_INPUT=0 reads it with zlib
   * instead): the time inside the inflater (a part of read_s), the members inflated on the device and the
   * compressed bytes read.  All zero for other input. */
  double inflate_s;
  uint64_t inflate_blocks, in_bytes;
} gwa_pipeline_stats_t;
int gwa_pipeline_open(gwa_index_t *const *ix, int n_ix, const gwa_config_t *cfg, uint32_t batch_reads,
                      int workers_per_device, gwa_pipeline_t **out);
/* SAM (no header) of any number of reads, in input order. */
int gwa_pipeline_align(gwa_pipeline_t *p, const gwa_reads_t *reads, gwa_results_t *out);
/* A FASTA / FASTQ file (.fa .fasta .fan .fastq .fq, optionally .gz or .snap; ReadReaderFactory.createReader,
 * R/ReadReaderFactory.java:126-151) streamed through the devices; SAM records (no header) are
 * written to fd in input order.  *n_reads = reads aligned.  A .gz file whose first member is a BGZF member
 * is inflated on the pipeline's first device, a chunk of whole members per kernel launch (BGZF input
 * above); a later member that is not BGZF, or a truncated last member, fails the run with its byte offset
 * (a missing EOF marker does not).  Any other .gz file is read with zlib on the IO thread.  The SAM is
 * byte for byte the plain file's either way.
 * A .bam file is read input too ("BAM input" above): it is a BGZF source like a .fastq.gz (GWA_BGZF_INPUT=0:
 * zlib; a first member that is not BGZF is an error), the reader consumes the header, walks the block_size
 * chain and cuts batches of records that are reads, and each batch's records are decoded on its device. */
int gwa_pipeline_align_file(gwa_pipeline_t *p, const char *path, int fd, uint64_t *n_reads);
/* The same over the bytes [begin, end) of a plain (not .gz / .snap / .bam) read file, which must start at a
 * record (gwa_reads_shard_range gives such ranges; it refuses a .bam as it refuses a .gz). */
int gwa_pipeline_align_file_range(gwa_pipeline_t *p, const char *path, int fd, uint64_t begin, uint64_t end,
                                  uint64_t *n_reads);
/* Paired-end read files streamed through the devices like gwa_pipeline_align_file: mate i of path1
 * pairs with mate i of path2; path2 == NULL means path1 is interleaved (records 2i and 2i + 1 form
 * pair i).  Each file may be FASTA or FASTQ, plain, .gz or .snap, independently of the other.  Two
 * SAM lines per pair (no header) are written to fd in pair order under the output rules above, byte
 * for byte what gwa_align_pairs gives for the same pairs; *n_pairs = pairs aligned, and
 * gwa_pipeline_stats_t.reads counts mates (two per pair).  batch_reads of gwa_pipeline_open counts
 * pairs here.  FASTQ mates go to HBM as text, both slices into one allocation, and are parsed there;
 * a batch with a FASTA mate is parsed on the host.  Host memory does not grow with the files: at most
 * `depth` pair batches are in flight, and the two files share the pinned-buffer budget of one.
 * flags: GWA_PAIR_CHECK_NAMES compares the mates' names (the parser's first whitespace-delimited
 * token, one trailing "/1" or "/2" removed from each; QNAME in the SAM is never altered) on the
 * device, and a differing pair fails the run with the lowest such pair index and both names.
 * Errors: -m sf and a bad insert range (as gwa_batch_create_pairs); mate files with different record
 * counts ("the mate files hold different numbers of reads"); an interleaved file with an odd record
 * count; a malformed record (the message starts with the file's name).  What was written to fd before
 * an error is unspecified.
 * BAM mates: two .bam files pair record i with record i (records that are reads; no flag check), and both are
 * decoded on the device in one allocation.  One .bam with path2 == NULL is interleaved: reads 2i and 2i + 1
 * form pair i, read 2i must carry FLAG 0x1 and 0x40 and read 2i + 1 FLAG 0x1 and 0x80; otherwise the run fails
 * naming the lowest such pair and both flags (a coordinate-sorted paired BAM fails this way rather than
 * pairing strangers).  A .bam beside a FASTQ or FASTA mate file is decoded by the host build, as a batch with
 * a FASTA mate is parsed on the host.  GWA_PAIR_CHECK_NAMES compares the names as they stand in the records. */
#define GWA_PAIR_CHECK_NAMES 1u
int gwa_pipeline_align_pair_files(gwa_pipeline_t *p, const char *path1, const char *path2, int32_t min_insert,
                                  int32_t max_insert, uint32_t flags, int fd, uint64_t *n_pairs);
/* The in-memory counterpart (as gwa_pipeline_align is of align_file): pairs of any number of mates,
 * dealt to the handles in batches of batch_reads pairs; results as gwa_align_pairs gives them
 * (paired = 1, n_reads = pairs, two lines per pair). */
int gwa_pipeline_align_pairs(gwa_pipeline_t *p, const gwa_reads_t *mate1, const gwa_reads_t *mate2, int32_t min_insert,
                             int32_t max_insert, gwa_results_t *out);
/* One process per GPU (C3; the reference's one read loop, A/Align.java:174-196, split by reads): the
 * byte range [*begin, *end) of shard `shard` of `nshards` contiguous shards of a plain FASTQ / FASTA
 * file, cut at record starts, so that the shards' SAM files concatenated in shard order equal a
 * one-process run's (the header belongs to shard 0). */
int gwa_reads_shard_range(const char *path, uint32_t shard, uint32_t nshards, uint64_t *begin, uint64_t *end);
/* The bytes of a `.snap` file (R/ReadReaderFactory.java:130-139, org.xerial.snappy.SnappyInputStream):
 * a snappy-java stream (magic header, then length-prefixed Snappy blocks) or one bare Snappy block,
 * decompressed into *out (malloc'd, NUL-terminated; gwa_free).  Host only, no device needed. */
int gwa_snappy_decompress(const uint8_t *in, uint64_t n, char **out, uint64_t *out_len);
/* What gwa_pipeline_align_file / _file_range / _pair_files write to fd from now on: GWA_OUT_SAM (the
 * default), GWA_OUT_BGZF -- each batch's SAM text as its own run of BGZF blocks (compressed on the
 * batch's device, one D2H of the blocks), in input order under the same pwrite / write rules; no header
 * and no EOF marker: the caller frames the file, as it writes the @SQ header -- or GWA_OUT_BAM: each
 * batch's BAM records as its own run of BGZF blocks under the same rules (the caller writes
 * BGZF(gwa_bam_header) before and the EOF marker after).  gwa_pipeline_align and
 * gwa_pipeline_align_pairs return text either way.  Another value fails ("gwa_pipeline_set_output:
 * unknown format N"). */
int gwa_pipeline_set_output(gwa_pipeline_t *p, uint32_t format);
/* Coordinate-sorted BAM ("Sorted BAM" above) from the file calls, from now on: valid only while the pipeline's
 * output is GWA_OUT_BAM.  Each gwa_pipeline_align_file / _file_range / _pair_files call is one sort scope: the
 * workers hand their batches to a run sorter (gwa_bam_sorter_add_batch with the batch's number, on the first
 * handle's device; tmp_dir and mem_bytes as gwa_bam_sorter_open takes them) instead of writing, and
 * gwa_bam_sorter_finish runs when the call ends: the sorted stream's blocks go to fd at its position, the
 * index to bai_fd (-1: none).  The caller writes BGZF(gwa_bam_header_sorted) before and the EOF marker after.
 * gwa_pipeline_sort_stats gives the sorter's counters and times of the last such call. */
int gwa_pipeline_set_sort(gwa_pipeline_t *p, const char *tmp_dir, uint64_t mem_bytes, int bai_fd);
int gwa_pipeline_sort_stats(const gwa_pipeline_t *p, gwa_bam_sorter_stats_t *st);
/* Duplicate marking ("Duplicate marking" above) in the sorted file calls from now on: valid only while the
 * pipeline sorts (gwa_pipeline_set_sort).  gwa_pipeline_markdup_stats gives the counts and times of the last
 * sorted call. */
int gwa_pipeline_set_markdup(gwa_pipeline_t *p, int on);
int gwa_pipeline_markdup_stats(const gwa_pipeline_t *p, gwa_markdup_stats_t *st);
int gwa_pipeline_stats(const gwa_pipeline_t *p, gwa_pipeline_stats_t *st);
void gwa_pipeline_close(gwa_pipeline_t *p);

#ifdef __cplusplus
}
#endif
#endif /* GWA_H */
