// record_stream.h -- a read file as a stream of slices of complete records (record_stream.cpp).
//
// Host code only (no HIP): the buffers come from an allocator the caller passes in, so the pipeline
// hands out its pooled pinned buffers and a stand-alone program plain malloc'd ones.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace gwa {

// A buffer of read-file text (pipeline.cpp BufPool owns and recycles them).
struct TextBuf {
  char *p = nullptr;
  size_t cap = 0, size = 0;
  bool pinned = false;
  const char *data() const { return p; }
};

// a buffer of at least `cap` bytes; the stream drops its reference once every slice cut from the
// buffer has been handed out
using TextAlloc = std::function<std::shared_ptr<TextBuf>(size_t cap)>;

namespace inflate {
struct Member;  // inflate_core.h: a BGZF member's payload and where its text goes
}
// Inflates the members m[0, n) of comp[0, compLen) (payload offsets relative to comp) to dst + outOff;
// dstLen = the sum of their ISIZEs.  Throws inflate::InflateError (inflate_host.h) for a member the
// decoder refuses.  The pipeline passes one that runs the kernel (inflate.hip); without one the stream
// uses the host build of the same decoder.
using Inflater = std::function<void(const uint8_t *comp, uint64_t compLen, const inflate::Member *m, uint64_t n,
                                    char *dst, uint64_t dstLen)>;

// 1: gzip (.gz, and .bam: a BAM file is a run of BGZF members), 2: snappy-java (.snap,
// R/ReadReaderFactory.java:130-139), 0: plain
int compressedKind(const char *path);
// 0: FASTA (.fa .fasta .fan), 1: FASTQ (.fastq .fq), below an optional .gz / .snap; 2: BAM (.bam); throws
// otherwise
int formatOf(const char *path);

// `n` complete records: the bytes [tb, te) of buf.  FASTQ: starts[k] = record k's header line,
// relative to tb (FASTA records are multi-line and parsed on the host, so their starts are not kept).
struct RecordSlice {
  std::shared_ptr<TextBuf> buf;
  uint64_t tb = 0, te = 0, n = 0;
  int format = 1;
  std::vector<uint64_t> starts;
  // BAM (format 2): [tb, te) is a run of whole alignment records, starts[k] = the k-th of them that is a
  // read (FLAG without 0x100 and 0x800; the others are skipped); the record at tb is record recIndex of the
  // file, at byte byteOff of its inflated stream (for error messages)
  uint64_t recIndex = 0, byteOff = 0;
};

// A .gz file whose first member is a BGZF member (a gzip member with the BC subfield) is a BGZF source,
// kind 3 (GWA_BGZF_INPUT=0 keeps it on the zlib path): the IO thread reads compressed bytes with pread,
// walks the members' headers, fills a chunk with whole members while their ISIZEs fit it and has them
// inflated by one call of the inflater.  Its chunks are at least 65 536 bytes, so any member fits one.  A
// later member that is not BGZF, and a truncated last member, are errors with the member's byte offset;
// a missing EOF marker is not.
//
// The file's records in order, in slices of exactly batchRecords records (the last one may be
// shorter).  An IO thread (started by the first next()) reads -- and decompresses -- the file in
// chunks into buffers from `alloc`, behind `reserve` bytes of room where the records carried over
// from the previous chunk are put; next() frames each chunk while the IO thread reads the following
// one.  Only full slices leave a chunk unless the file has ended; the rest carries over.
class RecordStream {
 public:
  // [begin, end): a byte range of a plain file that starts at a record (0, ~0: the whole file; a
  // compressed file takes no other).  chunkBytes = 0: 256 MB, or the file's size when it is smaller
  // (GWA_PIPE_CHUNK, a test knob, overrides both).
  RecordStream(const char *path, uint64_t begin, uint64_t end, uint64_t batchRecords, TextAlloc alloc,
               uint64_t chunkBytes = 0, Inflater inflater = nullptr);
  ~RecordStream();
  RecordStream(const RecordStream &) = delete;
  RecordStream &operator=(const RecordStream &) = delete;

  // the next slice; false at the end of the file.  Throws on a read error.
  bool next(RecordSlice *out);

  int format() const { return fmt_; }
  const std::string &path() const { return path_; }
  uint64_t chunk() const { return chunk_; }
  uint64_t reserve() const { return reserve_; }
  uint64_t bufBytes() const { return reserve_ + chunk_; }  // what the IO thread asks `alloc` for
  uint64_t fileBytes() const { return fileBytes_; }        // 0 = unknown (compressed, or not a regular file)
  double readSeconds();
  double frameSeconds() const { return frameS_; }
  // BGZF source: the time inside the inflater (a part of readSeconds), the members inflated by the
  // caller's inflater (0 with the host build) and the compressed bytes read
  bool bgzf() const { return kind_ == 3; }
  double inflateSeconds();
  uint64_t inflateBlocks();
  uint64_t compressedBytes();

 private:
  struct Chunk {
    std::shared_ptr<TextBuf> buf;
    uint64_t got = 0;
    bool final = false;
  };
  struct Source;  // the open file (plain descriptor, gzFile, SnapReader or BGZF state)
  void ioLoop();
  bool readBgzfChunk(char *dst, uint64_t chunk, uint64_t *got);  // true: the file has ended
  void stopIo();
  bool frameNextChunk();

  std::string path_;
  int fmt_ = 1, kind_ = 0;
  uint64_t begin_ = 0, end_ = ~0ull, batch_ = 1, chunk_ = 0, reserve_ = 0, fileBytes_ = 0;
  TextAlloc alloc_;
  Inflater inflater_;
  std::unique_ptr<Source> src_;
  // IO thread and its queue (at most two chunks read ahead)
  std::thread io_;
  std::mutex qmu_;
  std::condition_variable qcv_;
  std::deque<Chunk> q_;
  bool started_ = false, ioDone_ = false, stop_ = false;
  std::string ioErr_;
  double readS_ = 0, frameS_ = 0, inflateS_ = 0;
  uint64_t inflateBlocks_ = 0, compBytes_ = 0;
  // framing state: the records carried over, the slices of the current chunk not yet handed out
  std::shared_ptr<TextBuf> prev_;
  uint64_t carryFrom_ = 0, carryLen_ = 0;
  bool ended_ = false;
  std::deque<RecordSlice> ready_;
  std::vector<uint64_t> starts_;
  // BAM: whether the header has been consumed, and the record index and inflated-stream offset of the
  // first byte framed next (the carried records' first byte)
  bool bamHeaderDone_ = false;
  uint64_t bamRec_ = 0, bamByte_ = 0;
  uint64_t frameBam(const std::shared_ptr<TextBuf> &buf, uint64_t base, const char *t, uint64_t len, bool final);
};

// Paired-end input: two record streams, slice k of the one zipped with slice k of the other (the
// files differ in bytes per record, so each stream frames and carries on its own); or, with path2 ==
// nullptr, one stream of an interleaved file at twice the batch size (records 2i and 2i + 1 form pair
// i).  next() throws when the mate files hold different numbers of records -- either being the
// longer, by any count -- and when an interleaved file holds an odd number.
class PairedRecordStream {
 public:
  PairedRecordStream(const char *path1, const char *path2, uint64_t batchPairs, TextAlloc alloc, Inflater inflater = nullptr);
  // the next `*pairs` pairs: mate 1 in *m1 and mate 2 in *m2, or both alternating in *m1 (interleaved;
  // *m2 is left empty); false at the end of the input
  bool next(RecordSlice *m1, RecordSlice *m2, uint64_t *pairs);
  bool interleaved() const { return !b_; }
  std::vector<RecordStream *> streams();
  double readSeconds();
  double frameSeconds() const;

 private:
  std::unique_ptr<RecordStream> a_, b_;
};

}  // namespace gwa
