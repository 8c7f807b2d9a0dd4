// record_stream.cpp -- the pipeline's file reader and record framer (record_stream.h): host code
// only, shared by the single-end and the paired-end file entry points of pipeline.cpp.
#include "record_stream.h"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "bam_in_core.h"
#include "inflate_host.h"
#include "snappy_stream.h"

namespace gwa {
uint64_t frameRecords(const char *t, uint64_t len, int format, bool final, uint64_t maxRec, uint64_t *nRec,
                      std::vector<uint64_t> *starts);  // reads_io.cpp
void newlineCount(const char *t, uint64_t a, uint64_t b, uint64_t *count, bool *blank, bool *cr);
void recordStartsFromNewlines(const char *t, uint64_t a, uint64_t b, uint64_t g0, uint64_t *starts, uint64_t cap);

namespace {
using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// read-file chunks (and the room before each for the records carried over from the previous one);
// a smaller file reads in one chunk of its own size
constexpr uint64_t kChunk = 256ull << 20, kReserve = 512ull << 20;
// BGZF source: compressed bytes read per pread, and the largest member (BSIZE is 16 bits)
constexpr uint64_t kBgzfRead = 8ull << 20, kBgzfMember = 65536;
}  // namespace

int compressedKind(const char *path) {
  const size_t n = strlen(path);
  if (n > 3 && strcmp(path + n - 3, ".gz") == 0) return 1;
  if (n > 4 && strcmp(path + n - 4, ".bam") == 0) return 1;
  if (n > 5 && strcmp(path + n - 5, ".snap") == 0) return 2;
  return 0;
}

int formatOf(const char *path) {
  std::string s(path);
  if (s.size() > 3 && s.compare(s.size() - 3, 3, ".gz") == 0) s.resize(s.size() - 3);
  else if (s.size() > 5 && s.compare(s.size() - 5, 5, ".snap") == 0) s.resize(s.size() - 5);
  auto ends = [&](const char *x) {
    const size_t n = strlen(x);
    return s.size() >= n && s.compare(s.size() - n, n, x) == 0;
  };
  if (ends(".fa") || ends(".fasta") || ends(".fan")) return 0;
  if (ends(".fastq") || ends(".fq")) return 1;
  if (ends(".bam")) return 2;
  throw std::runtime_error(std::string("Unsupported file type: ") + path);
}

struct RecordStream::Source {
  gzFile f = nullptr;
  std::unique_ptr<SnapReader> snap;
  int in = -1;
  // BGZF: the file's bytes from offset cbufOff on that are not inflated yet, the next offset to read, the
  // members handed to the inflater so far
  std::vector<uint8_t> cbuf;
  uint64_t cbufOff = 0, fileAt = 0, members = 0;
  bool eof = false;
  ~Source() {
    if (f) gzclose(f);
    if (in >= 0) ::close(in);
  }
};

RecordStream::RecordStream(const char *path, uint64_t begin, uint64_t end, uint64_t batchRecords, TextAlloc alloc,
                           uint64_t chunkBytes, Inflater inflater)
    : path_(path), begin_(begin), end_(end), batch_(std::max<uint64_t>(1, batchRecords)), alloc_(std::move(alloc)),
      inflater_(std::move(inflater)), src_(new Source()) {
  fmt_ = formatOf(path);
  kind_ = compressedKind(path);
  const bool whole = begin == 0 && end == ~0ull;
  if (kind_) {
    if (!whole) throw std::runtime_error(std::string("a byte range needs an uncompressed read file: ") + path);
    if (kind_ == 1) {  // BGZF when the first member has the BC subfield (GWA_BGZF_INPUT=0: never)
      const char *e = getenv("GWA_BGZF_INPUT");
      if (!(e && e[0] == '0' && !e[1])) {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) throw std::runtime_error(std::string("cannot open ") + path);
        std::vector<uint8_t> head(kBgzfMember);
        uint64_t got = 0;
        for (;;) {
          const ssize_t r = ::pread(fd, head.data() + got, head.size() - got, (off_t)got);
          if (r <= 0) break;
          got += (uint64_t)r;
          if (got == head.size()) break;
        }
        inflate::Member m;
        uint32_t size = 0;
        std::string why;
        if (inflate::parseMember(head.data(), got, &m, &size, &why) == 1) {
          kind_ = 3;
          src_->in = fd;
        } else {
          ::close(fd);
          if (fmt_ == 2) throw std::runtime_error(std::string(path) + ": not a BAM file: the first BGZF member is missing (" +
                                                  (why.empty() ? std::string("the file ends inside it") : why) + ")");
        }
      }
    }
    if (kind_ == 1) {
      src_->f = gzopen(path, "rb");
      if (!src_->f) throw std::runtime_error(std::string("cannot open ") + path);
      gzbuffer(src_->f, 1u << 20);
    } else if (kind_ == 2) {
      src_->snap.reset(new SnapReader(path));
    }
  } else {
    src_->in = ::open(path, O_RDONLY);
    if (src_->in < 0) throw std::runtime_error(std::string("cannot open ") + path);
    struct stat st;
    const bool regular = ::fstat(src_->in, &st) == 0 && S_ISREG(st.st_mode);
    if (regular) end_ = std::min<uint64_t>(end_, (uint64_t)st.st_size);
    if (begin_ > end_) begin_ = end_;
    if (::lseek(src_->in, (off_t)begin_, SEEK_SET) < 0) throw std::runtime_error(std::string("cannot seek in ") + path);
    // chunk size: the whole file when it is smaller than kChunk (plain files; compressed sizes are unknown)
    if (regular) fileBytes_ = end_ - begin_;
  }
  chunk_ = fileBytes_ ? std::min<uint64_t>(kChunk, ((fileBytes_ >> 20) + 1) << 20) : kChunk;
  if (chunkBytes) chunk_ = chunkBytes;
  // GWA_PIPE_CHUNK (tests): chunk size in bytes, so that small files read in many chunks and take the
  // carry paths
  if (const char *e = getenv("GWA_PIPE_CHUNK"))
    if (strtoull(e, nullptr, 10) > 0) chunk_ = strtoull(e, nullptr, 10);
  if (kind_ == 3) chunk_ = std::max<uint64_t>(chunk_, kBgzfMember);  // (any member fits an empty chunk)
  reserve_ = std::min<uint64_t>(kReserve, 2 * chunk_);
}

RecordStream::~RecordStream() { stopIo(); }

void RecordStream::stopIo() {
  {
    std::lock_guard<std::mutex> g(qmu_);
    stop_ = true;
    qcv_.notify_all();
  }
  if (io_.joinable()) io_.join();
  q_.clear();
}

double RecordStream::readSeconds() {
  std::lock_guard<std::mutex> g(qmu_);
  return readS_;
}

double RecordStream::inflateSeconds() {
  std::lock_guard<std::mutex> g(qmu_);
  return inflateS_;
}
uint64_t RecordStream::inflateBlocks() {
  std::lock_guard<std::mutex> g(qmu_);
  return inflateBlocks_;
}
uint64_t RecordStream::compressedBytes() {
  std::lock_guard<std::mutex> g(qmu_);
  return compBytes_;
}

// BGZF source: whole members into dst while their ISIZEs fit `chunk`, inflated by one call
bool RecordStream::readBgzfChunk(char *dst, uint64_t chunk, uint64_t *got) {
  Source &S = *src_;
  std::vector<inflate::Member> ms;
  std::vector<uint64_t> offs;  // the members' offsets in the file
  uint64_t cur = 0, text = 0, readNow = 0;
  bool fileEnd = false;
  for (;;) {
    // a member is at most 65 536 bytes: with that many in the buffer, or the file's end, it is whole
    while (!S.eof && S.cbuf.size() - cur < kBgzfMember) {
      const size_t at = S.cbuf.size();
      S.cbuf.resize(at + kBgzfRead);
      const ssize_t r = ::pread(S.in, S.cbuf.data() + at, kBgzfRead, (off_t)S.fileAt);
      if (r < 0) throw std::runtime_error(std::string("read error: ") + path_);
      S.cbuf.resize(at + (size_t)r);
      S.fileAt += (uint64_t)r;
      readNow += (uint64_t)r;
      if (r == 0) S.eof = true;
    }
    const uint64_t avail = S.cbuf.size() - cur;
    if (avail == 0) {
      fileEnd = true;
      break;
    }
    inflate::Member m;
    uint32_t size = 0;
    std::string why;
    const int r = inflate::parseMember(S.cbuf.data() + cur, avail, &m, &size, &why);
    const std::string label = path_ + ": " + inflate::memberLabel(S.members + ms.size(), S.cbufOff + cur);
    if (r < 0) throw std::runtime_error(label + why);
    if (r == 0) throw std::runtime_error(label + "the file ends inside the member (" + std::to_string(avail) + " bytes left)");
    if (text + m.isize > chunk) break;
    m.payOff += cur;
    m.outOff = text;
    offs.push_back(S.cbufOff + cur);
    ms.push_back(m);
    text += m.isize;
    cur += size;
  }
  const auto t0 = Clock::now();
  try {
    if (inflater_) {
      inflater_(S.cbuf.data(), cur, ms.data(), ms.size(), dst, text);
    } else {
      std::vector<uint32_t> status(ms.size() + 1);
      const uint64_t bad = inflate::inflateHost(S.cbuf.data(), cur, ms.data(), ms.size(), (uint8_t *)dst, text, status.data());
      if (bad < ms.size()) throw inflate::InflateError(bad, status[bad]);
    }
  } catch (inflate::InflateError &e) {
    const uint64_t k = std::min<uint64_t>(e.member, ms.size() - 1);
    throw std::runtime_error(path_ + ": " + inflate::memberLabel(S.members + k, offs[k]) + e.what());
  }
  const double is = secs(t0, Clock::now());
  {
    std::lock_guard<std::mutex> g(qmu_);
    inflateS_ += is;
    if (inflater_) inflateBlocks_ += ms.size();
    compBytes_ += readNow;
  }
  S.cbuf.erase(S.cbuf.begin(), S.cbuf.begin() + (long)cur);
  S.cbufOff += cur;
  S.members += ms.size();
  *got = text;
  return fileEnd;
}

void RecordStream::ioLoop() {
  const uint64_t chunk = chunk_, reserve = reserve_, end = end_;
  const bool gz = kind_ != 0;
  const int in = src_->in;
  try {
    for (;;) {
      {
        std::unique_lock<std::mutex> g(qmu_);
        qcv_.wait(g, [&] { return stop_ || q_.size() < 2; });
        if (stop_) break;
      }
      Chunk c;
      c.buf = alloc_(reserve + chunk);
      const auto r0 = Clock::now();
      char *dst = c.buf->p + reserve;
      bool bgzfEnd = false;
      if (kind_ == 3) {
        bgzfEnd = readBgzfChunk(dst, chunk, &c.got);
      } else if (src_->snap) {
        c.got = src_->snap->read(dst, chunk);
      } else if (gz) {
        while (c.got < chunk) {
          const int r = gzread(src_->f, dst + c.got, (unsigned)std::min<uint64_t>(chunk - c.got, 1u << 30));
          if (r < 0) throw std::runtime_error(std::string("read error: ") + path_);
          if (r == 0) break;
          c.got += (uint64_t)r;
        }
      } else {  // four preads at a time (the page cache copies in parallel), up to `end`
        const off_t at = ::lseek(in, 0, SEEK_CUR);
        const uint64_t want = std::min<uint64_t>(chunk, end > (uint64_t)at ? end - (uint64_t)at : 0);
        std::atomic<bool> bad{false};
        std::vector<std::thread> th;
        std::vector<uint64_t> gotk(4, 0);
        auto lo = [&](int k) { return want * (uint64_t)k / 4; };
        for (int k = 0; k < 4; ++k)
          th.emplace_back([&, k] {
            const uint64_t part = lo(k + 1) - lo(k);
            uint64_t gk = 0;
            while (gk < part) {
              const ssize_t r = ::pread(in, dst + lo(k) + gk, (size_t)(part - gk), at + (off_t)(lo(k) + gk));
              if (r < 0) { bad = true; return; }
              if (r == 0) break;
              gk += (uint64_t)r;
            }
            gotk[(size_t)k] = gk;
          });
        for (auto &x : th) x.join();
        if (bad) throw std::runtime_error(std::string("read error: ") + path_);
        // the bytes read are contiguous up to the first short part (end of file)
        for (int k = 0; k < 4; ++k) {
          c.got += gotk[(size_t)k];
          if (gotk[(size_t)k] < lo(k + 1) - lo(k)) break;
        }
        ::lseek(in, at + (off_t)c.got, SEEK_SET);
        if ((uint64_t)at + c.got >= end) c.got = std::min<uint64_t>(c.got, end - (uint64_t)at);
      }
      // (a BGZF chunk ends before the member that does not fit: short, but not the file's last)
      c.final = kind_ == 3 ? bgzfEnd : c.got < chunk || (!gz && (uint64_t)::lseek(in, 0, SEEK_CUR) >= end);
      const double rs = secs(r0, Clock::now());
      std::lock_guard<std::mutex> g(qmu_);
      readS_ += rs;
      const bool fin = c.final;
      q_.push_back(std::move(c));
      qcv_.notify_all();
      if (fin) break;
    }
  } catch (std::exception &e) {
    std::lock_guard<std::mutex> g(qmu_);
    ioErr_ = e.what();
  }
  std::lock_guard<std::mutex> g(qmu_);
  ioDone_ = true;
  qcv_.notify_all();
}

// Frame the next chunk (behind the records carried over) into ready_; false when the file has ended.
bool RecordStream::frameNextChunk() {
  Chunk c;
  {
    std::unique_lock<std::mutex> g(qmu_);
    qcv_.wait(g, [&] { return !q_.empty() || ioDone_; });
    if (q_.empty()) {
      if (!ioErr_.empty()) throw std::runtime_error(ioErr_);
      return false;
    }
    c = std::move(q_.front());
    q_.pop_front();
    qcv_.notify_all();
  }
  const auto f0 = Clock::now();
  const uint64_t reserve = reserve_;
  const int fmt = fmt_;
  // the text of this round: the carried records, then the chunk
  std::shared_ptr<TextBuf> buf = c.buf;
  uint64_t base = reserve - std::min(reserve, carryLen_);
  if (carryLen_ > reserve) {  // more carry than room: one buffer holding both
    buf = alloc_(carryLen_ + c.got + 64);
    memcpy(buf->p + carryLen_, c.buf->p + reserve, c.got);
    base = 0;
  }
  if (carryLen_) memcpy(buf->p + base, prev_->p + carryFrom_, carryLen_);
  prev_.reset();
  const char *t = buf->p + base;
  const uint64_t len = carryLen_ + c.got;
  buf->size = base + len;
  const bool final = c.final;
  if (fmt == 2) {  // BAM: the header, then the block_size chain
    const uint64_t pos = frameBam(buf, base, t, len, final);
    frameS_ += secs(f0, Clock::now());
    if (final) {
      ended_ = true;
    } else {
      prev_ = buf;
      carryFrom_ = base + pos;
      carryLen_ = len - pos;
    }
    return true;
  }
  // all complete records of the text: their header offsets (FASTQ) and the end of the last
  std::vector<uint64_t> &starts = starts_;
  starts.clear();
  uint64_t nrec = 0, done = 0;
  bool fast = false;
  const unsigned nth = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  if (fmt == 1 && !final) {  // no '\r', no blank line: record k starts after newline 4k - 1
    std::vector<uint64_t> cnt(nth);
    std::vector<char> bl(nth), cr(nth);
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nth; ++k)
      th.emplace_back([&, k] {
        bool b0, c0;
        newlineCount(t, len * k / nth, len * (k + 1) / nth, &cnt[k], &b0, &c0);
        bl[k] = b0;
        cr[k] = c0;
      });
    for (auto &x : th) x.join();
    bool clean = len > 0 && t[0] != '\n';
    uint64_t tot = 0;
    std::vector<uint64_t> g0(nth);
    for (unsigned k = 0; k < nth; ++k) {
      clean = clean && !bl[k] && !cr[k];
      g0[k] = tot;
      tot += cnt[k];
    }
    if (clean) {
      fast = true;
      nrec = tot / 4;
      starts.resize(nrec + 1);
      starts[0] = 0;
      th.clear();
      for (unsigned k = 0; k < nth; ++k)
        th.emplace_back([&, k] {
          recordStartsFromNewlines(t, len * k / nth, len * (k + 1) / nth, g0[k], starts.data(), nrec + 1);
        });
      for (auto &x : th) x.join();
      done = starts[nrec];  // the start of the first incomplete record
      starts.resize(nrec);
    }
  }
  if (!fast) done = frameRecords(t, len, fmt, final, ~0ull, &nrec, fmt == 1 ? &starts : nullptr);
  // slices of batch_ records; the records after the last full slice carry over
  const uint64_t B = batch_;
  const uint64_t full = final ? (nrec + B - 1) / B : nrec / B;
  uint64_t pos = 0;
  if (fmt == 1) {
    for (uint64_t k = 0; k < full; ++k) {
      const uint64_t r0i = k * B, r1i = std::min(nrec, r0i + B);
      RecordSlice s;
      s.buf = buf;
      s.tb = base + starts[r0i];
      s.te = base + (r1i < nrec ? starts[r1i] : done);
      s.n = r1i - r0i;
      s.format = fmt;
      s.starts.assign(starts.begin() + (long)r0i, starts.begin() + (long)r1i);
      const uint64_t s0 = starts[r0i];
      for (auto &x : s.starts) x -= s0;
      ready_.push_back(std::move(s));
    }
    pos = (full * B < nrec) ? starts[full * B] : done;
  } else {  // FASTA: frame again slice by slice (record starts are not kept)
    uint64_t left = full == 0 ? 0 : nrec;
    while (left > 0) {
      uint64_t nr = 0;
      const uint64_t e = pos + frameRecords(t + pos, len - pos, fmt, final, std::min<uint64_t>(B, left), &nr, nullptr);
      if (nr == 0) break;
      if (nr < B && !final) break;
      RecordSlice s;
      s.buf = buf;
      s.tb = base + pos;
      s.te = base + e;
      s.n = nr;
      s.format = fmt;
      ready_.push_back(std::move(s));
      pos = e;
      left -= nr;
    }
  }
  frameS_ += secs(f0, Clock::now());
  if (final) {
    ended_ = true;
  } else {
    prev_ = buf;
    carryFrom_ = base + pos;
    carryLen_ = len - pos;
  }
  return true;
}

// BAM framing of the text t[0, len) (the carried bytes, then the chunk): the header first, which may take
// several chunks, then every whole record; slices of batch_ records that are reads.  Returns where the
// bytes to carry start: the first record that is not in a slice.
uint64_t RecordStream::frameBam(const std::shared_ptr<TextBuf> &buf, uint64_t base, const char *t, uint64_t len, bool final) {
  const uint8_t *u = (const uint8_t *)t;
  uint64_t at = 0;
  if (!bamHeaderDone_) {
    std::string why;
    const int64_t h = bamin::headerSize(u, len, &why);
    if (h == -2) throw std::runtime_error(path_ + ": " + why);
    if (h < 0) {
      if (final) throw std::runtime_error(path_ + ": the BAM header is cut off by the end of the file (" + std::to_string(len) + " bytes)");
      return 0;  // (all of it carries over)
    }
    bamHeaderDone_ = true;
    at = (uint64_t)h;
  }
  std::vector<uint64_t> &starts = starts_;
  std::vector<uint64_t> idx;
  starts.clear();
  uint64_t nAll = 0, done = 0;
  try {
    done = at + bamin::walkChain(u + at, len - at, final, bamRec_, bamByte_ + at, &starts, &idx, &nAll);
  } catch (std::exception &e) {
    throw std::runtime_error(path_ + ": " + e.what());
  }
  for (auto &x : starts) x += at;
  const uint64_t nrec = starts.size(), B = batch_;
  const uint64_t full = final ? (nrec + B - 1) / B : nrec / B;
  for (uint64_t k = 0; k < full; ++k) {
    const uint64_t r0i = k * B, r1i = std::min(nrec, r0i + B);
    RecordSlice s;
    s.buf = buf;
    s.tb = base + starts[r0i];
    s.te = base + (r1i < nrec ? starts[r1i] : done);
    s.n = r1i - r0i;
    s.format = 2;
    s.starts.assign(starts.begin() + (long)r0i, starts.begin() + (long)r1i);
    const uint64_t s0 = starts[r0i];
    for (auto &x : s.starts) x -= s0;
    s.recIndex = idx[r0i];
    s.byteOff = bamByte_ + s0;
    ready_.push_back(std::move(s));
  }
  const uint64_t pos = full * B < nrec ? starts[full * B] : done;
  bamRec_ = full * B < nrec ? idx[full * B] : bamRec_ + nAll;
  bamByte_ += pos;
  return pos;
}

bool RecordStream::next(RecordSlice *out) {
  if (!started_) {
    started_ = true;
    io_ = std::thread(&RecordStream::ioLoop, this);
  }
  while (ready_.empty()) {
    if (ended_ || !frameNextChunk()) {
      ended_ = true;
      return false;
    }
  }
  *out = std::move(ready_.front());
  ready_.pop_front();
  return true;
}

PairedRecordStream::PairedRecordStream(const char *path1, const char *path2, uint64_t batchPairs, TextAlloc alloc,
                                       Inflater inflater) {
  const uint64_t B = std::max<uint64_t>(1, batchPairs);
  a_.reset(new RecordStream(path1, 0, ~0ull, path2 ? B : 2 * B, alloc, 0, inflater));
  if (path2) b_.reset(new RecordStream(path2, 0, ~0ull, B, alloc, 0, inflater));
}

bool PairedRecordStream::next(RecordSlice *m1, RecordSlice *m2, uint64_t *pairs) {
  const bool h1 = a_->next(m1);
  if (!b_) {
    if (!h1) return false;
    if (m1->n % 2) throw std::runtime_error("the interleaved file holds an odd number of reads: " + a_->path());
    *m2 = RecordSlice();
    *pairs = m1->n / 2;
    return true;
  }
  const bool h2 = b_->next(m2);
  if (!h1 && !h2) return false;
  // every slice but a stream's last holds exactly the batch size, so unequal files show here: as
  // slices of different sizes, or as one stream ending a slice before the other
  if (!h1 || !h2 || m1->n != m2->n) throw std::runtime_error("the mate files hold different numbers of reads");
  *pairs = m1->n;
  return true;
}

std::vector<RecordStream *> PairedRecordStream::streams() {
  std::vector<RecordStream *> v{a_.get()};
  if (b_) v.push_back(b_.get());
  return v;
}

double PairedRecordStream::readSeconds() { return a_->readSeconds() + (b_ ? b_->readSeconds() : 0.0); }
double PairedRecordStream::frameSeconds() const { return a_->frameSeconds() + (b_ ? b_->frameSeconds() : 0.0); }

}  // namespace gwa
