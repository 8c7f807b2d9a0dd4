// pipeline.cpp -- the multi-device, overlapped host driver of the align path (include/gwa.h
// gwa_pipeline_*).
//
// The reference aligns one read at a time on one thread and emits each SAM line as it goes
// (A/Align.java:174-196, PassReadToAligner; A/SAMOutput.java:53 autoflush).  Here reads are cut into
// batches that are dealt to every device handle as it becomes free -- each handle is a full index
// replica on its own GPU, so there is no exchange between devices (reads shard embarrassingly) --
// and the SAM of the batches is written back in input order, byte-identical to a one-device run.
//
// Threads: one reader (the file: framing of complete records only, no parsing), W workers per
// device (parse a framed slice, set the batch up on the device, run the kernels, format the SAM),
// and the caller, which writes the results in batch order.  The workers of one device run their
// batches' kernels concurrently, each batch on its own stream and search scratch (gwa_api.cpp
// Scratch), so one batch's set-up, deep-tier tail and SAM formatting overlap another's kernels.  At
// most `depth` batches are in flight, which bounds memory.
//
// Paired-end input takes the same route with pair batches: two mate files (or one interleaved file)
// are read and framed by record_stream.cpp, which zips slice k of the one with slice k of the other;
// a worker puts both slices' FASTQ text into one device allocation (gwa_api.cpp
// batchCreatePairsFastq) and the batch's SAM holds two lines per pair.
#include <hip/hip_runtime.h>

#include "bam_in_core.h"
#include "record_stream.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "../../include/gwa.h"

extern "C" int gwa_fail_message(const char *msg);  // gwa_api.cpp

namespace gwa {
void checkSamTags(uint32_t tags);
int batchCreateFastq(gwa_index_t *ix, const gwa_config_t *cfg, const char *text, uint64_t len, const uint64_t *start,
                     uint32_t n, gwa_batch_t **out);
// a paired batch from the mates' FASTQ text: two segments, or (text2 == nullptr) one interleaved
// segment whose start1 holds the np mate-1 starts and then the np mate-2 starts (gwa_api.cpp)
int batchCreatePairsFastq(gwa_index_t *ix, const gwa_config_t *cfg, const char *text1, uint64_t len1,
                          const uint64_t *start1, const char *text2, uint64_t len2, const uint64_t *start2, uint32_t np,
                          int32_t minInsert, int32_t maxInsert, const char *label1, const char *label2,
                          gwa_batch_t **out);
// BAM input (gwa_api.cpp): a batch from the framed records of a BAM slice, decoded on the device; the paired
// form takes two segments, or (bytes2 == nullptr) one interleaved segment whose start1 holds the np mate-1
// starts and then the np mate-2 starts; and the host build of the decoder over one slice
int batchCreateBam(gwa_index_t *ix, const gwa_config_t *cfg, const uint8_t *bytes, uint64_t len, const uint64_t *start,
                   uint32_t n, uint64_t recIndex, uint64_t byteOff, const char *label, gwa_batch_t **out);
int batchCreatePairsBam(gwa_index_t *ix, const gwa_config_t *cfg, const uint8_t *bytes1, uint64_t len1, const uint64_t *start1,
                        uint64_t recIndex1, uint64_t byteOff1, const uint8_t *bytes2, uint64_t len2, const uint64_t *start2,
                        uint64_t recIndex2, uint64_t byteOff2, uint32_t np, int32_t minInsert, int32_t maxInsert,
                        const char *label1, const char *label2, gwa_batch_t **out);
int bamDecodeHostSlice(const uint8_t *bytes, uint64_t len, uint64_t recIndex, uint64_t byteOff, const char *label,
                       gwa_read_buf_t *out);
// the lowest pair of a paired batch whose mate names differ (false: none)
bool batchMateNamesDiffer(gwa_batch_t *b, uint32_t *pair, std::string *name1, std::string *name2);
uint64_t batchSamInto(gwa_batch_t *b, char **buf, uint64_t *cap);  // gwa_api.cpp
uint64_t batchBgzfInto(gwa_batch_t *b, char **buf, uint64_t *cap);  // the same as BGZF blocks
uint64_t batchBamInto(gwa_batch_t *b, char **buf, uint64_t *cap);   // the batch's BAM records as BGZF blocks
void pinnedFree(char *p);
char *pinnedAlloc(uint64_t bytes);
// BGZF read files: the kernel path of the inflater (inflate.hip), on the device of an index handle
namespace inflate {
struct Member;
}
struct DeviceInflater;
DeviceInflater *inflaterCreate(int device);
void inflaterFree(DeviceInflater *d);
void inflaterRun(DeviceInflater *d, const uint8_t *comp, uint64_t n, const inflate::Member *ms, uint64_t nm, uint8_t *dst,
                 uint64_t dstLen, int repeat);
int indexDevice(const gwa_index_t *ix);  // gwa_api.cpp
}

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// Read-file text lives in pooled buffers (record_stream.h TextBuf).  Pinned host memory makes the
// batch's H2D copy one DMA instead of a
// staged pageable copy, which the runtime serialises across worker threads (measured: set-up 0.36 s
// -> 0.21 s and 11 -> 22 M reads/s FASTQ -> SAM for 10M reads).  Pinning takes about a second per
// 5 GB; gwa_pipeline_open pins the buffers a run keeps in flight, and the pool falls back to pageable
// buffers beyond them.  Buffers are recycled when the last job that references one is done, and kept
// across align_file calls.
using gwa::TextBuf;
using gwa::compressedKind;
using gwa::formatOf;

class BufPool {
  std::mutex mu;
  std::vector<TextBuf *> free_, freePageable_;
  std::shared_ptr<bool> alive = std::make_shared<bool>(true);  // buffers out at destruction free themselves

  static void release(TextBuf *b) {
    if (b->pinned) gwa::pinnedFree(b->p);
    else ::free(b->p);
    delete b;
  }
  static TextBuf *take(std::vector<TextBuf *> &v, size_t cap) {
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i]->cap >= cap) {
        TextBuf *b = v[i];
        v.erase(v.begin() + (long)i);
        return b;
      }
    return nullptr;
  }

 public:
  ~BufPool() {
    std::lock_guard<std::mutex> g(mu);
    *alive = false;
    for (auto *b : free_) release(b);
    for (auto *b : freePageable_) release(b);
    free_.clear();
    freePageable_.clear();
  }
  // a pinned buffer for the free list (the background pinning thread)
  void addPinned(size_t cap) {
    TextBuf *b = new TextBuf();
    try {
      b->p = gwa::pinnedAlloc(cap);
    } catch (...) {
      delete b;
      throw;
    }
    b->cap = cap;
    b->pinned = true;
    std::lock_guard<std::mutex> g(mu);
    if (!*alive) { release(b); return; }
    free_.push_back(b);
    // a pageable buffer is dropped for each pinned one that arrives
    if (!freePageable_.empty()) {
      release(freePageable_.back());
      freePageable_.pop_back();
    }
  }
  // free pinned buffers of at least `cap` bytes
  uint64_t countPinned(size_t cap) {
    std::lock_guard<std::mutex> g(mu);
    uint64_t n = 0;
    for (auto *b : free_) n += b->cap >= cap ? 1 : 0;
    return n;
  }
  // unpin the free pinned buffers smaller than `cap` (they can never serve a request of that size);
  // returns how many and their bytes
  void releasePinnedBelow(size_t cap, uint64_t *n, uint64_t *bytes) {
    std::lock_guard<std::mutex> g(mu);
    *n = *bytes = 0;
    for (size_t i = 0; i < free_.size();)
      if (free_[i]->cap < cap) {
        ++*n;
        *bytes += free_[i]->cap;
        release(free_[i]);
        free_.erase(free_.begin() + (long)i);
      } else {
        ++i;
      }
  }
  std::shared_ptr<TextBuf> get(size_t cap) {
    TextBuf *b = nullptr;
    {
      std::lock_guard<std::mutex> g(mu);
      b = take(free_, cap);
      if (!b) b = take(freePageable_, cap);
    }
    if (!b) {
      b = new TextBuf();
      b->p = (char *)::malloc(cap);
      if (!b->p) {
        delete b;
        throw std::runtime_error("out of host memory for the read text");
      }
      b->cap = cap;
    }
    b->size = 0;
    std::shared_ptr<bool> live = alive;
    return std::shared_ptr<TextBuf>(b, [this, live](TextBuf *x) {
      if (!*live) { release(x); return; }
      std::lock_guard<std::mutex> g(mu);
      (x->pinned ? free_ : freePageable_).push_back(x);
    });
  }
};

// One unit of work: either reads already in memory (a gwa_reads_t slice) or a framed slice of file
// text that the worker parses itself.
struct Job {
  uint64_t id = 0;
  gwa_reads_t reads{};                 // in-memory reads (text == nullptr)
  std::shared_ptr<TextBuf> text;       // or: file text holding complete records [tb, te)
  uint64_t tb = 0, te = 0;
  int format = 1;
  std::vector<uint64_t> starts;  // FASTQ: each record's header line, relative to tb
  // paired-end (pairs > 0): mate 1 above, mate 2 here -- in-memory reads, or a second slice of file
  // text; an interleaved slice has no second text and holds the mates alternating (2 * pairs records)
  uint64_t pairs = 0;
  gwa_reads_t reads2{};
  std::shared_ptr<TextBuf> text2;
  uint64_t tb2 = 0, te2 = 0;
  int format2 = 1;
  std::vector<uint64_t> starts2;
  // BAM slices (format 2): where their first record stands in the file (RecordSlice), and the file's name
  uint64_t recIndex = 0, byteOff = 0, recIndex2 = 0, byteOff2 = 0;
  std::string label;
};

// a run's paired-end parameters (gwa_pipeline_align_pair_files / gwa_pipeline_align_pairs)
struct PairSetup {
  int32_t minInsert = 0, maxInsert = 0;
  bool checkNames = false;
  std::string label1, label2;  // the mate files, for error messages
};

// host copies of one mate set's reads (the mates of an interleaved FASTA slice, taken apart)
struct HostReads {
  std::string name, seq, qual;
  std::vector<uint64_t> nameOff{0}, seqOff{0}, qualOff{0};
  bool hasQual = false;
  void add(const gwa_reads_t &r, uint32_t i) {
    name.append(r.name + r.name_off[i], r.name_off[i + 1] - r.name_off[i]);
    seq.append(r.seq + r.seq_off[i], r.seq_off[i + 1] - r.seq_off[i]);
    nameOff.push_back(name.size());
    seqOff.push_back(seq.size());
    if (r.qual) {
      hasQual = true;
      qual.append(r.qual + r.qual_off[i], r.qual_off[i + 1] - r.qual_off[i]);
      qualOff.push_back(qual.size());
    }
  }
  gwa_reads_t view() const {
    gwa_reads_t v{};
    v.n = (uint32_t)(nameOff.size() - 1);
    v.name = name.data();
    v.seq = seq.data();
    v.name_off = nameOff.data();
    v.seq_off = seqOff.data();
    if (hasQual) {
      v.qual = qual.data();
      v.qual_off = qualOff.data();
    }
    return v;
  }
};

struct Result {
  gwa_results_t r{};
  uint32_t n = 0;
};

}  // namespace

namespace {
// MemAvailable of /proc/meminfo in bytes (0 = unknown)
uint64_t memAvailable() {
  FILE *f = fopen("/proc/meminfo", "r");
  if (!f) return 0;
  char line[256];
  uint64_t kb = 0;
  while (fgets(line, sizeof line, f))
    if (sscanf(line, "MemAvailable: %lu kB", (unsigned long *)&kb) == 1) break;
  fclose(f);
  return kb * 1024;
}
}  // namespace

struct gwa_pipeline {
  std::vector<gwa_index_t *> ix;
  gwa_config_t cfg{};
  uint32_t batchReads = 1u << 20;
  int workersPerDevice = 2;
  gwa_pipeline_stats_t stats{};
  uint32_t outFormat = GWA_OUT_SAM;  // what file runs write (gwa_pipeline_set_output)
  // coordinate-sorted BAM (gwa_pipeline_set_sort): every file call is one sort scope
  bool sortOn = false, sortHasTmp = false;
  std::string sortTmp;
  uint64_t sortMem = 0;
  int sortBaiFd = -1;
  gwa_bam_sorter_stats_t sortStats{};  // of the last sorted call
  bool markdupOn = false;                // duplicate marking in the sort scope (gwa_pipeline_set_markdup)
  gwa_markdup_stats_t markdupStats{};    // of the last sorted call
  BufPool pool;  // pinned read-text buffers, kept across align_file calls
  uint64_t pinnedBufs = 0, pinnedBytes = 0;  // pinned so far (lazily, by align_file)
  std::mutex samMu;
  std::vector<std::pair<char *, uint64_t>> samBufs;  // pinned SAM buffers, one per file worker, kept too
  // BGZF read files are inflated on the first handle's device, on a stream of the inflater's own with
  // pooled device buffers; made by the first chunk that needs it, kept across align_file calls
  std::mutex inflaterMu;
  gwa::DeviceInflater *inflater = nullptr;
  gwa::Inflater deviceInflater() {
    return [this](const uint8_t *comp, uint64_t n, const gwa::inflate::Member *ms, uint64_t nm, char *dst, uint64_t dstLen) {
      {
        std::lock_guard<std::mutex> g(inflaterMu);
        if (!inflater) inflater = gwa::inflaterCreate(gwa::indexDevice(ix[0]));
      }
      gwa::inflaterRun(inflater, comp, n, ms, nm, (uint8_t *)dst, dstLen, 1);
    };
  }
  ~gwa_pipeline() {
    for (auto &b : samBufs) gwa::pinnedFree(b.first);
    if (inflater) gwa::inflaterFree(inflater);
  }
};

namespace {

// the run sorter of one sorted file call (closed with the run)
struct SorterHold {
  gwa_bam_sorter_t *s = nullptr;
  ~SorterHold() {
    if (s) gwa_bam_sorter_close(s);
  }
};

// Shared state of one run (align or align_file).
struct Run {
  gwa_pipeline *p;
  SorterHold sort;  // set: the workers add their batches to it instead of writing
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  std::map<uint64_t, Result> done;
  bool noMoreJobs = false, failed = false;
  std::string err;
  size_t inflight = 0, depth;
  std::vector<std::thread> workers;
  std::atomic<uint64_t> reads{0};
  std::vector<double> devBusy;  // per device: seconds of kernels
  double parseS = 0, setupS = 0, formatS = 0, writeS = 0, waitS = 0;  // summed over worker threads
  // file mode: each worker writes its own batch's SAM from its pinned buffer -- at its offset with
  // pwrite when the output is a regular file (offsets fixed in batch order as sizes become known),
  // else in batch order with write
  int fd = -1;
  bool seekable = false;
  uint64_t base = 0;                        // file position of the first record
  std::map<uint64_t, uint64_t> sizes, offs; // batch -> SAM bytes / offset
  uint64_t cursor = 0, nextOff = 0;         // first batch whose offset is not fixed yet, its offset
  uint64_t turn = 0;                        // non-seekable output: the batch that writes next
  std::atomic<uint64_t> fileReads{0}, fileBatches{0}, outBytes{0};
  // paired-end runs.  A mate-name mismatch (GWA_PAIR_CHECK_NAMES) does not fail the run at once: the
  // batches before it, which are all with their workers by then, finish first, so that the pair
  // reported is the lowest of the whole input whatever order the batches complete in.
  const PairSetup *pair = nullptr;
  uint64_t nameFailId = ~0ull;  // lowest batch with a mismatch
  std::string nameErr;

  explicit Run(gwa_pipeline *p_) : p(p_) {
    depth = std::max<size_t>(4, 2 * p->ix.size() * p->workersPerDevice);
    devBusy.assign(p->ix.size(), 0.0);
  }

  void fail(const std::string &m) {
    std::lock_guard<std::mutex> g(mu);
    if (!failed) { failed = true; err = m; }
    cv.notify_all();
  }

  // producer side: blocks while `depth` batches are in flight; false once the run has failed
  bool push(Job &&j) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return failed || nameFailId != ~0ull || inflight < depth; });
    if (failed || nameFailId != ~0ull) return false;
    ++inflight;
    jobs.push_back(std::move(j));
    cv.notify_all();
    return true;
  }
  void finishJobs() {
    std::lock_guard<std::mutex> g(mu);
    noMoreJobs = true;
    cv.notify_all();
  }

  void worker(int d) {
    gwa_index_t *ix = p->ix[(size_t)d];
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return failed || !jobs.empty() || noMoreJobs; });
        if (failed || jobs.empty()) return;
        j = std::move(jobs.front());
        jobs.pop_front();
      }
      Result res;
      gwa_read_buf_t parsed{};
      const gwa_reads_t *rd = &j.reads;
      int rc = 0;
      if (j.text) {
        uint64_t used = 0;
        rc = gwa_reads_parse(j.text->data() + j.tb, j.te - j.tb, j.format, 1, &parsed, &used);
        rd = &parsed.reads;
      }
      if (rc == 0) {
        res.n = rd->n;
        gwa_batch_t *b = nullptr;
        rc = j.pairs ? gwa_batch_create_pairs(ix, &p->cfg, rd, &j.reads2, pair->minInsert, pair->maxInsert, &b)
                     : gwa_batch_create(ix, &p->cfg, rd, &b);
        if (rc == 0) {
          const auto t0 = Clock::now();
          rc = gwa_batch_run(b);
          const double kt = secs(t0, Clock::now());
          if (rc == 0) rc = gwa_batch_results(b, &res.r);
          {
            std::lock_guard<std::mutex> g(mu);
            devBusy[(size_t)d] += kt;
          }
        }
        gwa_batch_free(b);
      }
      const std::string msg = rc != 0 ? std::string(gwa_last_error()) : std::string();
      if (j.text) gwa_reads_free(&parsed);
      if (rc != 0) {
        gwa_results_free(&res.r);
        fail("batch " + std::to_string(j.id) + " on device handle " + std::to_string(d) + ": " + msg);
        return;
      }
      reads += res.n;
      std::lock_guard<std::mutex> g(mu);
      done.emplace(j.id, std::move(res));
      cv.notify_all();
    }
  }

  // file mode: put batch `id`'s SAM (size bytes at p) into the output in batch order
  void output(uint64_t id, const char *p, uint64_t size) {
    const auto w0 = Clock::now();
    uint64_t off = 0;
    {
      std::unique_lock<std::mutex> g(mu);
      if (seekable) {
        sizes[id] = size;
        for (auto it = sizes.find(cursor); it != sizes.end(); it = sizes.find(cursor)) {
          offs[cursor] = nextOff;
          nextOff += it->second;
          sizes.erase(it);
          ++cursor;
        }
        cv.notify_all();
        cv.wait(g, [&] { return failed || nameFailId < id || offs.count(id) != 0; });
        if (failed || nameFailId < id) return;
        off = offs[id];
        offs.erase(id);
      } else {
        cv.wait(g, [&] { return failed || nameFailId < id || turn == id; });
        if (failed || nameFailId < id) return;
      }
    }
    const auto w1 = Clock::now();
    uint64_t done = 0;
    while (done < size) {
      const size_t chunk = (size_t)std::min<uint64_t>(size - done, 1ull << 30);
      const ssize_t w = seekable ? ::pwrite(fd, p + done, chunk, (off_t)(base + off + done)) : ::write(fd, p + done, chunk);
      if (w <= 0) throw std::runtime_error("write to the SAM output failed");
      done += (uint64_t)w;
    }
    const auto w2 = Clock::now();
    std::lock_guard<std::mutex> g(mu);
    if (!seekable) ++turn;
    waitS += secs(w0, w1);
    writeS += secs(w1, w2);
    cv.notify_all();
  }

  // file mode worker: parse its framed slice, align it on device d, write its SAM
  void fileWorker(int d) {
    gwa_index_t *ix = p->ix[(size_t)d];
    char *pinned = nullptr;
    uint64_t cap = 0;
    {
      std::lock_guard<std::mutex> g(p->samMu);
      if (!p->samBufs.empty()) {
        pinned = p->samBufs.back().first;
        cap = p->samBufs.back().second;
        p->samBufs.pop_back();
      }
    }
    try {
      for (;;) {
        Job j;
        {
          std::unique_lock<std::mutex> g(mu);
          cv.wait(g, [&] { return failed || !jobs.empty() || noMoreJobs; });
          if (failed || jobs.empty()) break;
          j = std::move(jobs.front());
          jobs.pop_front();
          if (j.id > nameFailId) {  // (a batch after a mate-name mismatch: not run)
            --inflight;
            cv.notify_all();
            continue;
          }
        }
        const auto t0 = Clock::now();
        gwa_batch_t *b = nullptr;
        int rc = 0;
        uint32_t nr = 0;
        auto t1 = t0;
        if (j.pairs) {
          nr = (uint32_t)(2 * j.pairs);
          rc = createPairBatch(ix, j, &b, &t1);
          if (rc == 0 && pair->checkNames) {
            uint32_t at = 0;
            std::string n1, n2;
            bool differ = false;
            try {
              differ = gwa::batchMateNamesDiffer(b, &at, &n1, &n2);
            } catch (...) {
              gwa_batch_free(b);
              throw;
            }
            if (differ) {
              gwa_batch_free(b);
              std::lock_guard<std::mutex> g(mu);
              if (j.id < nameFailId) {
                nameFailId = j.id;
                nameErr = "the mate names of pair " + std::to_string(j.id * p->batchReads + at) + " differ: '" + n1 +
                          "' and '" + n2 + "'";
              }
              --inflight;
              cv.notify_all();
              continue;
            }
          }
        } else if (j.format == 1) {  // FASTQ: the text itself goes to the device, fields located there
          nr = (uint32_t)j.starts.size();
          rc = gwa::batchCreateFastq(ix, &p->cfg, j.text->data() + j.tb, j.te - j.tb, j.starts.data(), nr, &b);
        } else if (j.format == 2) {  // BAM: the records go to the device and are decoded there
          nr = (uint32_t)j.starts.size();
          rc = gwa::batchCreateBam(ix, &p->cfg, (const uint8_t *)j.text->data() + j.tb, j.te - j.tb, j.starts.data(), nr,
                                   j.recIndex, j.byteOff, j.label.c_str(), &b);
        } else {  // FASTA reads (multi-line records): parsed on the host
          gwa_read_buf_t parsed{};
          uint64_t used = 0;
          if (gwa_reads_parse(j.text->data() + j.tb, j.te - j.tb, j.format, 1, &parsed, &used) != 0)
            throw std::runtime_error(gwa_last_error());
          t1 = Clock::now();
          nr = parsed.reads.n;
          rc = gwa_batch_create(ix, &p->cfg, &parsed.reads, &b);
          gwa_reads_free(&parsed);
        }
        j.text.reset();
        j.text2.reset();
        const auto t2 = Clock::now();
        if (rc == 0) rc = gwa_batch_run(b);
        const auto t3 = Clock::now();
        uint64_t size = 0;
        if (rc == 0 && sort.s) {
          rc = gwa_bam_sorter_add_batch(sort.s, j.id, b);
        } else if (rc == 0) {
          try {
            size = p->outFormat == GWA_OUT_BAM    ? gwa::batchBamInto(b, &pinned, &cap)
                   : p->outFormat == GWA_OUT_BGZF ? gwa::batchBgzfInto(b, &pinned, &cap)
                                                  : gwa::batchSamInto(b, &pinned, &cap);
          } catch (...) {
            gwa_batch_free(b);
            throw;
          }
        }
        const std::string msg = rc != 0 ? std::string(gwa_last_error()) : std::string();
        gwa_batch_free(b);
        if (rc != 0) throw std::runtime_error("batch " + std::to_string(j.id) + ": " + msg);
        const auto t4 = Clock::now();
        if (!sort.s) output(j.id, pinned, size);
        outBytes += size;
        fileReads += nr;
        ++fileBatches;
        std::lock_guard<std::mutex> g(mu);
        parseS += secs(t0, t1);
        setupS += secs(t1, t2);
        devBusy[(size_t)d] += secs(t2, t3);
        formatS += secs(t3, t4);
        --inflight;
        cv.notify_all();
      }
    } catch (std::exception &e) {
      fail(e.what());
    }
    if (pinned) {
      std::lock_guard<std::mutex> g(p->samMu);
      p->samBufs.emplace_back(pinned, cap);
    }
  }

  // a paired batch from a job's two slices (or its one interleaved slice): FASTQ text goes to the
  // device as it is; with a FASTA mate both slices are parsed on the host, as single-end FASTA is
  int createPairBatch(gwa_index_t *ix, Job &j, gwa_batch_t **b, Clock::time_point *parsed) {
    const uint32_t np = (uint32_t)j.pairs;
    const char *t1 = j.text->data() + j.tb;
    const bool inter = !j.text2;
    if (j.format == 2 && (inter || j.format2 == 2)) {  // BAM mates: decoded on the device
      const uint8_t *u1 = (const uint8_t *)t1;
      if (inter) {  // mate-1 starts (even records), then mate-2 starts
        std::vector<uint64_t> st(2 * (size_t)np);
        for (uint32_t i = 0; i < np; ++i) {
          st[i] = j.starts[2 * (size_t)i];
          st[(size_t)np + i] = j.starts[2 * (size_t)i + 1];
        }
        return gwa::batchCreatePairsBam(ix, &p->cfg, u1, j.te - j.tb, st.data(), j.recIndex, j.byteOff, nullptr, 0, nullptr, 0,
                                        0, np, pair->minInsert, pair->maxInsert, pair->label1.c_str(), nullptr, b);
      }
      return gwa::batchCreatePairsBam(ix, &p->cfg, u1, j.te - j.tb, j.starts.data(), j.recIndex, j.byteOff,
                                      (const uint8_t *)j.text2->data() + j.tb2, j.te2 - j.tb2, j.starts2.data(), j.recIndex2,
                                      j.byteOff2, np, pair->minInsert, pair->maxInsert, pair->label1.c_str(),
                                      pair->label2.c_str(), b);
    }
    if (j.format == 1 && (inter || j.format2 == 1)) {
      if (inter) {  // mate-1 starts (even records), then mate-2 starts
        std::vector<uint64_t> st(2 * (size_t)np);
        for (uint32_t i = 0; i < np; ++i) {
          st[i] = j.starts[2 * (size_t)i];
          st[(size_t)np + i] = j.starts[2 * (size_t)i + 1];
        }
        return gwa::batchCreatePairsFastq(ix, &p->cfg, t1, j.te - j.tb, st.data(), nullptr, 0, nullptr, np,
                                          pair->minInsert, pair->maxInsert, pair->label1.c_str(), nullptr, b);
      }
      return gwa::batchCreatePairsFastq(ix, &p->cfg, t1, j.te - j.tb, j.starts.data(), j.text2->data() + j.tb2,
                                        j.te2 - j.tb2, j.starts2.data(), np, pair->minInsert, pair->maxInsert,
                                        pair->label1.c_str(), pair->label2.c_str(), b);
    }
    gwa_read_buf_t p1{}, p2{};
    uint64_t used = 0;
    int rc = 0;
    // (a BAM slice beside a FASTQ or FASTA mate: the host build of the decoder; its messages name the file)
    auto parse = [&](const char *t, uint64_t len, int fmt, uint64_t recIndex, uint64_t byteOff, const std::string &label,
                     gwa_read_buf_t *o) {
      if (fmt == 2) {
        if (gwa::bamDecodeHostSlice((const uint8_t *)t, len, recIndex, byteOff, label.c_str(), o) != 0)
          throw std::runtime_error(gwa_last_error());
      } else if (gwa_reads_parse(t, len, fmt, 1, o, &used) != 0) {
        throw std::runtime_error(label + ": " + gwa_last_error());
      }
    };
    try {
      parse(t1, j.te - j.tb, j.format, j.recIndex, j.byteOff, pair->label1, &p1);
      if (inter) {
        if (p1.reads.n != 2 * np) throw std::runtime_error(pair->label1 + ": the records of a batch do not parse as framed");
        HostReads m1, m2;
        for (uint32_t i = 0; i < np; ++i) {
          m1.add(p1.reads, 2 * i);
          m2.add(p1.reads, 2 * i + 1);
        }
        *parsed = Clock::now();
        const gwa_reads_t v1 = m1.view(), v2 = m2.view();
        rc = gwa_batch_create_pairs(ix, &p->cfg, &v1, &v2, pair->minInsert, pair->maxInsert, b);
      } else {
        parse(j.text2->data() + j.tb2, j.te2 - j.tb2, j.format2, j.recIndex2, j.byteOff2, pair->label2, &p2);
        *parsed = Clock::now();
        rc = gwa_batch_create_pairs(ix, &p->cfg, &p1.reads, &p2.reads, pair->minInsert, pair->maxInsert, b);
      }
    } catch (...) {
      gwa_reads_free(&p1);
      gwa_reads_free(&p2);
      throw;
    }
    gwa_reads_free(&p1);
    gwa_reads_free(&p2);
    return rc;
  }

  void startFile() {
    for (int w = 0; w < p->workersPerDevice; ++w)
      for (size_t d = 0; d < p->ix.size(); ++d) workers.emplace_back(&Run::fileWorker, this, (int)d);
  }

  void start() {
    for (int w = 0; w < p->workersPerDevice; ++w)
      for (size_t d = 0; d < p->ix.size(); ++d) workers.emplace_back(&Run::worker, this, (int)d);
  }

  // consumer side: the result of batch `id` (blocks); false once the run has failed
  bool take(uint64_t id, Result *out) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return failed || done.count(id) != 0; });
    if (failed) return false;
    auto it = done.find(id);
    *out = std::move(it->second);
    done.erase(it);
    --inflight;
    cv.notify_all();
    return true;
  }

  void join() {
    finishJobs();
    for (auto &t : workers) t.join();
    workers.clear();
    for (auto &kv : done) gwa_results_free(&kv.second.r);
    done.clear();
  }
};

// The first record start at or after byte x of a plain read file of `size` bytes (size when none):
// FASTA, a line starting with '>'; FASTQ, a line starting with '@' whose next-but-one line starts
// with '+'.  The FASTQ test is unique: a quality line may start with '@', but two lines below it is
// the next record's sequence line (or header), never a '+' line; sequence lines start with neither.
// A record found this way is one the sequential framing (frameRecords) starts as well.
uint64_t syncRecord(int fd, uint64_t size, uint64_t x, int fmt) {
  if (x == 0 || x >= size) return x >= size ? size : 0;
  uint64_t win = 1ull << 20;
  for (;;) {
    const uint64_t a = x - 1, b = std::min(size, a + win);
    std::string t(b - a, '\0');
    uint64_t got = 0;
    while (got < t.size()) {
      const ssize_t r = ::pread(fd, &t[got], t.size() - got, (off_t)(a + got));
      if (r <= 0) throw std::runtime_error("read error while locating a shard boundary");
      got += (uint64_t)r;
    }
    const bool atEnd = b == size;
    // line starts from x on: x itself when byte x - 1 ends a line
    size_t p = 1;
    if (t[0] != '\n') {
      const size_t nl = t.find('\n', 1);
      if (nl == std::string::npos) {
        if (atEnd) return size;
        win *= 4;
        continue;
      }
      p = nl + 1;
    }
    bool more = false;
    while (p < t.size()) {
      if (fmt == 0 ? t[p] == '>' : t[p] == '@') {
        if (fmt == 0) return a + p;
        const size_t n1 = t.find('\n', p), n2 = n1 == std::string::npos ? n1 : t.find('\n', n1 + 1);
        if (n2 == std::string::npos || n2 + 1 >= t.size()) {
          if (atEnd) return size;  // no complete record follows
          more = true;
          break;
        }
        if (t[n2 + 1] == '+') return a + p;
      }
      const size_t nl = t.find('\n', p);
      if (nl == std::string::npos) {
        if (atEnd) return size;
        more = true;
        break;
      }
      p = nl + 1;
    }
    if (!more && atEnd) return size;
    win *= 4;
  }
}

}  // namespace

extern "C" {

int gwa_pipeline_open(gwa_index_t *const *ix, int n_ix, const gwa_config_t *cfg, uint32_t batch_reads,
                      int workers_per_device, gwa_pipeline_t **out) {
  try {
    if (n_ix < 1) throw std::runtime_error("gwa_pipeline_open: no index handle");
    if (cfg->strategy < 0 || cfg->strategy > 3) throw std::runtime_error("unknown strategy");
    gwa::checkSamTags(cfg->sam_tags);
    auto *p = new gwa_pipeline();
    p->ix.assign(ix, ix + n_ix);
    p->cfg = *cfg;
    p->batchReads = batch_reads ? batch_reads : (1u << 20);
    p->workersPerDevice = workers_per_device > 0 ? workers_per_device : 3;
    *out = p;
    return 0;
  } catch (std::exception &e) {
    return gwa_fail_message(e.what());
  }
}

void gwa_pipeline_close(gwa_pipeline_t *p) { delete p; }

int gwa_pipeline_set_output(gwa_pipeline_t *p, uint32_t format) {
  if (format != GWA_OUT_SAM && format != GWA_OUT_BGZF && format != GWA_OUT_BAM)
    return gwa_fail_message(("gwa_pipeline_set_output: unknown format " + std::to_string(format) +
                             " (GWA_OUT_SAM = 0, GWA_OUT_BGZF = 1, GWA_OUT_BAM = 2)").c_str());
  p->outFormat = format;
  return 0;
}

int gwa_pipeline_set_sort(gwa_pipeline_t *p, const char *tmp_dir, uint64_t mem_bytes, int bai_fd) {
  if (p->outFormat != GWA_OUT_BAM)
    return gwa_fail_message("gwa_pipeline_set_sort: sorting needs a pipeline whose output is BAM (gwa_pipeline_set_output "
                            "GWA_OUT_BAM)");
  p->sortOn = true;
  p->sortHasTmp = tmp_dir != nullptr;
  p->sortTmp = tmp_dir ? tmp_dir : "";
  p->sortMem = mem_bytes;
  p->sortBaiFd = bai_fd;
  return 0;
}

int gwa_pipeline_set_markdup(gwa_pipeline_t *p, int on) {
  if (!p->sortOn)
    return gwa_fail_message("gwa_pipeline_set_markdup: duplicate marking needs a pipeline that sorts (gwa_pipeline_set_sort)");
  p->markdupOn = on != 0;
  return 0;
}

int gwa_pipeline_markdup_stats(const gwa_pipeline_t *p, gwa_markdup_stats_t *st) {
  *st = p->markdupStats;
  return 0;
}

int gwa_pipeline_sort_stats(const gwa_pipeline_t *p, gwa_bam_sorter_stats_t *st) {
  *st = p->sortStats;
  return 0;
}

int gwa_pipeline_stats(const gwa_pipeline_t *p, gwa_pipeline_stats_t *st) {
  *st = p->stats;
  return 0;
}

}  // extern "C"

namespace {

// reads [a, a + c) of a caller's gwa_reads_t
gwa_reads_t sliceReads(const gwa_reads_t *reads, uint32_t a, uint32_t c) {
  gwa_reads_t s = *reads;
  s.n = c;
  s.name_off = reads->name_off + a;
  s.seq_off = reads->seq_off + a;
  s.qual_off = reads->qual ? reads->qual_off + a : nullptr;
  s.qual_null = reads->qual && reads->qual_null ? reads->qual_null + a : nullptr;
  return s;
}

// what gwa_batch_create_pairs refuses, refused before a run starts
void checkPairRun(const gwa_config_t &cfg, int32_t minInsert, int32_t maxInsert) {
  if (cfg.strategy != 0) throw std::runtime_error("paired-end alignment runs the -m bsf search");
  if (minInsert < 0 || maxInsert < minInsert) throw std::runtime_error("bad insert-size range");
}

// gwa_pipeline_align (mate2 == nullptr) and gwa_pipeline_align_pairs (units = pairs)
int alignInMemory(gwa_pipeline_t *p, const gwa_reads_t *reads, const gwa_reads_t *mate2, const PairSetup *pair,
                  gwa_results_t *out) {
  Run run(p);
  run.pair = pair;
  std::thread feeder;
  try {
    const auto t0 = Clock::now();
    const uint32_t n = reads->n;
    const uint64_t nb = ((uint64_t)n + p->batchReads - 1) / p->batchReads;
    run.start();
    feeder = std::thread([&] {
      for (uint64_t i = 0; i < nb; ++i) {
        Job j;
        j.id = i;
        const uint32_t a = (uint32_t)(i * p->batchReads), c = (uint32_t)std::min<uint64_t>(p->batchReads, n - a);
        j.reads = sliceReads(reads, a, c);
        if (mate2) {
          j.pairs = c;
          j.reads2 = sliceReads(mate2, a, c);
        }
        if (!run.push(std::move(j))) break;
      }
      run.finishJobs();
    });
    std::vector<Result> parts;
    bool ok = true;
    for (uint64_t i = 0; i < nb && ok; ++i) {
      Result r;
      ok = run.take(i, &r);
      if (ok) parts.push_back(std::move(r));
    }
    feeder.join();
    run.join();
    if (!ok) {
      for (auto &r : parts) gwa_results_free(&r.r);
      throw std::runtime_error(run.err);
    }
    uint64_t total = 0;
    for (auto &r : parts) total += r.r.sam_len;
    out->n_reads = n;
    out->records = nullptr;
    out->n_records = 0;
    out->paired = mate2 ? 1 : 0;
    out->sam = (char *)malloc(total + 1);
    out->sam_len = total;
    out->line_off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)n + 1));
    uint64_t pos = 0, ri = 0;
    for (auto &r : parts) {
      memcpy(out->sam + pos, r.r.sam, r.r.sam_len);
      for (uint32_t k = 0; k < r.r.n_reads; ++k) out->line_off[ri++] = pos + r.r.line_off[k];
      pos += r.r.sam_len;
      gwa_results_free(&r.r);
    }
    out->line_off[n] = pos;
    out->sam[total] = 0;
    p->stats = gwa_pipeline_stats_t{};
    p->stats.reads = mate2 ? 2 * (uint64_t)n : n;
    p->stats.batches = nb;
    p->stats.wall_s = secs(t0, Clock::now());
    p->stats.read_s = 0;
    for (size_t d = 0; d < p->ix.size() && d < 16; ++d) p->stats.device_kernel_s[d] = run.devBusy[d];
    return 0;
  } catch (std::exception &e) {
    run.fail(e.what());  // (wakes a feeder blocked in push)
    if (feeder.joinable()) feeder.join();
    run.join();
    return gwa_fail_message(e.what());
  }
}

}  // namespace

extern "C" {

int gwa_pipeline_align(gwa_pipeline_t *p, const gwa_reads_t *reads, gwa_results_t *out) {
  return alignInMemory(p, reads, nullptr, nullptr, out);
}

int gwa_pipeline_align_pairs(gwa_pipeline_t *p, const gwa_reads_t *mate1, const gwa_reads_t *mate2, int32_t min_insert,
                             int32_t max_insert, gwa_results_t *out) {
  try {
    if (mate1->n != mate2->n) throw std::runtime_error("paired-end: the mate files hold different numbers of reads");
    checkPairRun(p->cfg, min_insert, max_insert);
  } catch (std::exception &e) {
    return gwa_fail_message(e.what());
  }
  PairSetup ps;
  ps.minInsert = min_insert;
  ps.maxInsert = max_insert;
  return alignInMemory(p, mate1, mate2, &ps, out);
}

int gwa_reads_shard_range(const char *path, uint32_t shard, uint32_t nshards, uint64_t *begin, uint64_t *end) {
  int in = -1;
  try {
    if (nshards == 0 || shard >= nshards) throw std::runtime_error("shard index out of range");
    const int fmt = formatOf(path);
    if (compressedKind(path))
      throw std::runtime_error(std::string("a sharded run needs an uncompressed read file (not .gz / .snap): ") + path);
    in = ::open(path, O_RDONLY);
    if (in < 0) throw std::runtime_error(std::string("cannot open ") + path);
    struct stat st;
    if (::fstat(in, &st) != 0 || !S_ISREG(st.st_mode))
      throw std::runtime_error(std::string("a sharded run needs a regular read file: ") + path);
    const uint64_t size = (uint64_t)st.st_size;
    auto cut = [&](uint64_t s) -> uint64_t {
      if (s == 0) return 0;
      if (s >= nshards) return size;
      return syncRecord(in, size, (uint64_t)((unsigned __int128)size * s / nshards), fmt);
    };
    *begin = cut(shard);
    *end = cut(shard + 1);
    ::close(in);
    return 0;
  } catch (std::exception &e) {
    if (in >= 0) ::close(in);
    return gwa_fail_message(e.what());
  }
}

int gwa_pipeline_align_file(gwa_pipeline_t *p, const char *path, int fd, uint64_t *n_reads) {
  return gwa_pipeline_align_file_range(p, path, fd, 0, ~0ull, n_reads);
}

}  // extern "C"

namespace {

// where a file run's SAM goes: batches are written at their offsets (pwrite) only to a regular file
// opened without O_APPEND -- pwrite ignores the offset under O_APPEND (Linux) and would append in
// completion order
void setOutput(Run &run, int fd) {
  struct stat sb;
  const off_t pos0 = ::lseek(fd, 0, SEEK_CUR);
  run.fd = fd;
  const int fl = ::fcntl(fd, F_GETFL);
  run.seekable = pos0 >= 0 && fl >= 0 && !(fl & O_APPEND) && ::fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
  run.base = run.seekable ? (uint64_t)pos0 : 0;
  gwa_pipeline *p = run.p;
  if (p->sortOn) {  // a sort scope: the workers hand their batches to the sorter, finishFileRun writes
    if (p->outFormat != GWA_OUT_BAM) throw std::runtime_error("gwa_pipeline_set_sort: sorting needs BAM output (GWA_OUT_BAM)");
    if (gwa_bam_sorter_open(p->ix[0], gwa::indexDevice(p->ix[0]), p->sortHasTmp ? p->sortTmp.c_str() : nullptr, p->sortMem,
                            &run.sort.s) != 0)
      throw std::runtime_error(gwa_last_error());
    if (p->markdupOn && gwa_bam_sorter_set_markdup(run.sort.s, 1) != 0) throw std::runtime_error(gwa_last_error());
  }
}

// Pin the read-text buffers a run keeps in flight (read-ahead, the chunk being framed, the batches in
// the workers) before it starts -- pinning while batches run stalls their copies in the runtime
// (measured: FASTQ -> SAM 8 M reads/s with background pinning, 20-25 M with the buffers pinned
// first) -- as many as the streams need, at most a quarter of the available host memory (one budget
// for all the streams of a run), kept for later calls.  Beyond them runs use pageable buffers.
// Buffers pinned by an earlier call for a smaller file cannot hold this run's chunks: they are
// unpinned, and only the pinned buffers of at least bufCap bytes count.  Returns those.
uint64_t pinReadBuffers(gwa_pipeline *p, const std::vector<gwa::RecordStream *> &streams) {
  const uint64_t nbuf = 4 + (uint64_t)p->ix.size() * (uint64_t)p->workersPerDevice;
  uint64_t need = 0, bufCap = 0;
  for (const gwa::RecordStream *s : streams) {
    need += s->fileBytes() ? std::min<uint64_t>(nbuf, s->fileBytes() / s->chunk() + 3) : nbuf;
    bufCap = std::max(bufCap, s->bufBytes());
  }
  const uint64_t avail = memAvailable(), capB = avail ? avail / 4 : (8ull << 30);
  uint64_t relN = 0, relB = 0;
  p->pool.releasePinnedBelow(bufCap, &relN, &relB);
  p->pinnedBufs -= std::min(p->pinnedBufs, relN);
  p->pinnedBytes -= std::min(p->pinnedBytes, relB);
  uint64_t usable = p->pool.countPinned(bufCap);
  try {
    while (usable < need && p->pinnedBytes + bufCap <= capB) {
      p->pool.addPinned(bufCap);
      ++p->pinnedBufs;
      ++usable;
      p->pinnedBytes += bufCap;
    }
  } catch (std::exception &) {  // (pinning failed: pageable buffers)
  }
  return usable;
}

// the end of a file run: workers joined, the output position, the counters
void finishFileRun(gwa_pipeline *p, Run &run, int fd, Clock::time_point t0, double readS, double frameS,
                   uint64_t pinnedUsable, const std::vector<gwa::RecordStream *> &streams) {
  run.finishJobs();
  for (auto &t : run.workers) t.join();
  run.workers.clear();
  if (run.failed) throw std::runtime_error(run.err);
  if (run.nameFailId != ~0ull) throw std::runtime_error(run.nameErr);
  if (run.seekable) ::lseek(fd, (off_t)(run.base + run.nextOff), SEEK_SET);
  if (run.sort.s) {  // the sorted stream's blocks, then the index
    p->sortStats = gwa_bam_sorter_stats_t{};
    if (gwa_bam_sorter_finish(run.sort.s, fd, p->sortBaiFd, &p->sortStats) != 0) throw std::runtime_error(gwa_last_error());
    run.outBytes += p->sortStats.out_bytes;
    p->markdupStats = gwa_markdup_stats_t{};
    (void)gwa_bam_sorter_markdup_stats(run.sort.s, &p->markdupStats);
  }
  gwa_pipeline_stats_t &st = p->stats;
  st = gwa_pipeline_stats_t{};
  st.reads = run.fileReads;
  st.batches = run.fileBatches;
  st.pinned_bufs = pinnedUsable;
  st.wall_s = secs(t0, Clock::now());
  st.read_s = readS;
  st.frame_s = frameS;
  for (size_t d = 0; d < p->ix.size() && d < 16; ++d) st.device_kernel_s[d] = run.devBusy[d];
  st.parse_s = run.parseS;
  st.setup_s = run.setupS;
  st.format_s = run.formatS;
  st.write_s = run.writeS;
  st.order_wait_s = run.waitS;
  st.out_bytes = run.outBytes;
  for (gwa::RecordStream *rs : streams) {
    st.inflate_s += rs->inflateSeconds();
    st.inflate_blocks += rs->inflateBlocks();
    st.in_bytes += rs->compressedBytes();
  }
}

}  // namespace

extern "C" {

int gwa_pipeline_align_file_range(gwa_pipeline_t *p, const char *path, int fd, uint64_t begin, uint64_t end,
                                  uint64_t *n_reads) {
  Run run(p);
  try {
    // The stream's IO thread reads the file in chunks into pooled pinned buffers and this thread
    // frames them into batches of complete records (record_stream.cpp); the workers do the rest.
    gwa::RecordStream rs(path, begin, end, p->batchReads, [p](size_t cap) { return p->pool.get(cap); }, 0,
                         p->deviceInflater());
    setOutput(run, fd);
    const uint64_t pinnedUsable = pinReadBuffers(p, {&rs});
    const auto t0 = Clock::now();
    run.startFile();
    gwa::RecordSlice s;
    uint64_t id = 0;
    while (rs.next(&s)) {
      Job j;
      j.id = id++;
      j.text = std::move(s.buf);
      j.tb = s.tb;
      j.te = s.te;
      j.format = s.format;
      j.starts = std::move(s.starts);
      j.recIndex = s.recIndex;
      j.byteOff = s.byteOff;
      if (s.format == 2) j.label = path;
      if (!run.push(std::move(j))) break;
    }
    finishFileRun(p, run, fd, t0, rs.readSeconds(), rs.frameSeconds(), pinnedUsable, {&rs});
    if (n_reads) *n_reads = run.fileReads;
    return 0;
  } catch (std::exception &e) {
    run.fail(e.what());
    run.join();
    return gwa_fail_message(e.what());
  }
}

int gwa_pipeline_align_pair_files(gwa_pipeline_t *p, const char *path1, const char *path2, int32_t min_insert,
                                  int32_t max_insert, uint32_t flags, int fd, uint64_t *n_pairs) {
  Run run(p);
  PairSetup ps;
  try {
    checkPairRun(p->cfg, min_insert, max_insert);
    if (flags & ~(uint32_t)GWA_PAIR_CHECK_NAMES) throw std::runtime_error("gwa_pipeline_align_pair_files: unknown flag");
    ps.minInsert = min_insert;
    ps.maxInsert = max_insert;
    ps.checkNames = (flags & GWA_PAIR_CHECK_NAMES) != 0;
    ps.label1 = path1;
    ps.label2 = path2 ? path2 : path1;
    run.pair = &ps;
    // The two mate files as zipped record streams, or one interleaved file (record_stream.cpp
    // PairedRecordStream); both streams draw their buffers from the pipeline's pool.
    const bool inter = path2 == nullptr;
    gwa::PairedRecordStream prs(path1, path2, p->batchReads, [p](size_t cap) { return p->pool.get(cap); },
                                p->deviceInflater());
    setOutput(run, fd);
    const uint64_t pinnedUsable = pinReadBuffers(p, prs.streams());
    const auto t0 = Clock::now();
    run.startFile();
    gwa::RecordSlice s1, s2;
    uint64_t id = 0, np = 0;
    while (prs.next(&s1, &s2, &np)) {
      Job j;
      j.id = id++;
      j.pairs = np;
      j.text = std::move(s1.buf);
      j.tb = s1.tb;
      j.te = s1.te;
      j.format = s1.format;
      j.starts = std::move(s1.starts);
      j.recIndex = s1.recIndex;
      j.byteOff = s1.byteOff;
      // an interleaved BAM: the mate flags, checked here in input order so that the lowest pair is named
      if (inter && j.format == 2)
        gwa::bamin::checkMateFlags((const uint8_t *)j.text->data() + j.tb, j.starts.data(), np, (id - 1) * (uint64_t)p->batchReads);
      if (!inter) {
        j.text2 = std::move(s2.buf);
        j.tb2 = s2.tb;
        j.te2 = s2.te;
        j.format2 = s2.format;
        j.starts2 = std::move(s2.starts);
        j.recIndex2 = s2.recIndex;
        j.byteOff2 = s2.byteOff;
      }
      if (!run.push(std::move(j))) break;
    }
    finishFileRun(p, run, fd, t0, prs.readSeconds(), prs.frameSeconds(), pinnedUsable, prs.streams());
    if (n_pairs) *n_pairs = run.fileReads / 2;
    return 0;
  } catch (std::exception &e) {
    run.fail(e.what());
    run.join();
    return gwa_fail_message(e.what());
  }
}

}  // extern "C"
