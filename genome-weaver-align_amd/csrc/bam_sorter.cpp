// bam_sorter.cpp -- the run sorter of the coordinate-sorted BAM output (bam_sorter.h; the rules: include/gwa.h).
#include "bam_sorter.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#ifdef GWA_BAM_SORT_HOST_ONLY
#include "bgzf_host.h"
#else
#include "../../include/gwa.h"
#include "bam_dup.h"
#include "bam_sort.h"
#endif

namespace gwa {

using namespace bamsort;
using bamdup::BamDupInfo;

namespace {
double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void writeAll(int fd, const uint8_t *p, uint64_t n, const char *what) {
  while (n) {
    const ssize_t w = ::write(fd, p, n > (1u << 30) ? (1u << 30) : (size_t)n);
    if (w < 0) {
      if (errno == EINTR) continue;
      throw std::runtime_error(std::string("gwa_bam_sorter: writing ") + what + ": " + strerror(errno));
    }
    p += w;
    n -= (uint64_t)w;
  }
}
// BGZF blocks of in[0, n) appended to out
void compressPart(int device, const uint8_t *in, uint64_t n, std::vector<uint8_t> &out) {
  out.clear();
  if (!n) return;
#ifdef GWA_BAM_SORT_HOST_ONLY
  (void)device;
  bgzf::compressHost(in, n, out);
#else
  uint8_t *p = nullptr;
  uint64_t len = 0;
  if (gwa_bgzf_compress(device, in, n, &p, &len) != 0) throw std::runtime_error(gwa_last_error());
  out.assign(p, p + len);
  gwa_free(p);
#endif
}
}  // namespace

BamSorter::BamSorter(std::vector<std::string> names, std::vector<int64_t> lengths, int device, const char *tmpDir, uint64_t memBytes)
    : names_(std::move(names)), lengths_(std::move(lengths)), device_(device), haveTmp_(tmpDir != nullptr),
      tmpDir_(tmpDir ? tmpDir : ""), memBytes_(memBytes) {
#ifdef GWA_BAM_SORT_HOST_ONLY
  if (device >= 0) throw std::runtime_error("gwa_bam_sorter: this build has no device");
#endif
  if (haveTmp_) {
    struct stat sb;
    if (stat(tmpDir_.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
      throw std::runtime_error("gwa_bam_sorter: tmp_dir " + tmpDir_ + " is not a directory");
  }
}

void BamSorter::dropRuns() {
  for (auto &r : runs_)
    if (!r.second.path.empty()) (void)unlink(r.second.path.c_str());
  runs_.clear();
  memUsed_ = 0;
}

BamSorter::~BamSorter() { dropRuns(); }

void BamSorter::addRecords(uint64_t runId, const uint8_t *bytes, uint64_t len) {
  const std::vector<uint64_t> off = validateChain(bytes, len);
  const uint64_t n = off.size() - 1;
  std::vector<uint8_t> sorted;
  std::vector<BamRecInfo> info;
  std::vector<BamDupInfo> dup;
  const bool md = markdup_;
  double dupS = 0;
#ifndef GWA_BAM_SORT_HOST_ONLY
  if (device_ >= 0) {
    sorted.resize(len);
    info.resize(n);
    if (md) dup.resize(n);
    bamSortBytesDevice(device_, bytes, off.data(), n, sorted.data(), info.data(), md ? dup.data() : nullptr, &dupS);
  } else
#endif
  {
    std::vector<uint64_t> perm;
    sortHost(bytes, off.data(), n, sorted, info, md ? &perm : nullptr);
    if (md) {
      const double t0 = now();
      std::vector<BamDupInfo> in;
      bamdup::runHost(bytes, off.data(), n, in);
      dup.resize(n);
      for (uint64_t i = 0; i < n; ++i) dup[i] = in[perm[i]];
      dupS = now() - t0;
    }
  }
  if (md) {
    addDupSeconds(dupS);
    addSortedRun(runId, std::move(sorted), std::move(info), std::move(dup));
  } else {
    addSortedRun(runId, std::move(sorted), std::move(info));
  }
}

void BamSorter::setMarkdup(bool on) {
  std::lock_guard<std::mutex> g(mu_);
  if (added_) throw std::runtime_error("gwa_bam_sorter_set_markdup: duplicate marking is set before the first run is added");
  markdup_ = on;
}

void BamSorter::addSortedRun(uint64_t runId, std::vector<uint8_t> &&sorted, std::vector<BamRecInfo> &&info) {
  addSortedRun(runId, std::move(sorted), std::move(info), std::vector<BamDupInfo>());
}

void BamSorter::addSortedRun(uint64_t runId, std::vector<uint8_t> &&sorted, std::vector<BamRecInfo> &&info,
                             std::vector<BamDupInfo> &&dup) {
  const double t0 = now();
  Run run;
  run.len = sorted.size();
  run.info = std::move(info);
  if (markdup_) {  // the run's templates: its distinct leaders (every one a record of the run)
    const uint64_t n = run.info.size();
    if (dup.size() != n)
      throw std::runtime_error("gwa_bam_sorter: run " + std::to_string(runId) + " has " + std::to_string(n) + " records and " +
                               std::to_string(dup.size()) + " duplicate-marking entries");
    std::vector<uint8_t> seen(n, 0);
    for (const BamDupInfo &x : dup) {
      if (x.leader >= n) throw std::runtime_error("gwa_bam_sorter: run " + std::to_string(runId) + " names a template leader outside the run");
      run.templates += !seen[x.leader];
      seen[x.leader] = 1;
    }
    run.dup = std::move(dup);
  }
  bool spill = false;
  {
    std::lock_guard<std::mutex> g(mu_);
    added_ = true;
    if (runs_.count(runId)) throw std::runtime_error("gwa_bam_sorter: run " + std::to_string(runId) + " was added twice");
    if (run.len && (memUsed_ + run.len > memBytes_ || memUsed_ + run.len < memUsed_)) {
      if (!haveTmp_)
        throw std::runtime_error("gwa_bam_sorter: run " + std::to_string(runId) + " of " + std::to_string(run.len) +
                                 " bytes does not fit mem_bytes " + std::to_string(memBytes_) + " (" + std::to_string(memUsed_) +
                                 " in use) and no tmp_dir was given");
      spill = true;
      char name[96];
      snprintf(name, sizeof name, "/gwa_sort_%ld_%p_%llu.run", (long)getpid(), (void *)this, (unsigned long long)serial_++);
      run.path = tmpDir_ + name;
    } else {
      memUsed_ += run.len;
    }
    runs_[runId] = Run{};  // (the id is taken; filled below)
  }
  try {
    if (spill) {
      const int fd = open(run.path.c_str(), O_CREAT | O_EXCL | O_WRONLY | O_CLOEXEC, 0600);
      if (fd < 0) throw std::runtime_error("gwa_bam_sorter: cannot create " + run.path + ": " + strerror(errno));
      try {
        writeAll(fd, sorted.data(), sorted.size(), "a spilled run");
      } catch (...) {
        (void)close(fd);
        (void)unlink(run.path.c_str());
        throw;
      }
      if (close(fd) != 0) {
        (void)unlink(run.path.c_str());
        throw std::runtime_error("gwa_bam_sorter: closing " + run.path + ": " + strerror(errno));
      }
    } else {
      run.bytes = std::move(sorted);
    }
  } catch (...) {
    std::lock_guard<std::mutex> g(mu_);
    runs_.erase(runId);
    throw;
  }
  std::lock_guard<std::mutex> g(mu_);
  st_.records += run.info.size();
  st_.bytes += run.len;
  ++st_.runs;
  if (spill) {
    ++st_.spilled_runs;
    st_.spilled_bytes += run.len;
  }
  runs_[runId] = std::move(run);
  st_.add_s += now() - t0;
}

void BamSorter::finish(int fdBam, int fdBai, BamSorterStats *stOut) {
  std::lock_guard<std::mutex> g(mu_);
  struct Cursor {
    Run *run = nullptr;
    FILE *f = nullptr;
    uint64_t next = 0, off = 0;
  };
  std::vector<Cursor> cur;
  bamdup::DupStats ds;
  auto closeAll = [&]() {
    for (auto &c : cur)
      if (c.f) fclose(c.f);
    cur.clear();
  };
  try {
    int64_t H = 0;
    if (fdBai >= 0) {
      for (size_t i = 0; i < lengths_.size(); ++i)
        if (lengths_[i] > kMaxEnd)
          throw std::runtime_error("gwa_bam_sorter: contig " + names_[i] + " has " + std::to_string(lengths_[i]) +
                                   " bases; a .bai index covers at most " + std::to_string(kMaxEnd) + " (2^29) per contig");
      H = (int64_t)lseek(fdBam, 0, SEEK_CUR);
      if (H < 0)
        throw std::runtime_error("gwa_bam_sorter: an index needs the stream's place in the BAM file, and the BAM descriptor "
                                 "is not seekable (a pipe?)");
    }
    // 1. the order of all records: run-major ordinals, stably sorted by key
    double t = now();
    std::vector<uint64_t> runStart;
    uint64_t N = 0;
    for (auto &r : runs_) {
      runStart.push_back(N);
      N += r.second.info.size();
      Cursor c;
      c.run = &r.second;
      cur.push_back(c);
    }
    if (N > 0xFFFFFFFEull) throw std::runtime_error("gwa_bam_sorter: more than 2^32 - 2 records in one sort scope");
    std::vector<uint32_t> perm(N);
    {
      std::vector<uint64_t> keys(N);
      uint64_t at = 0;
      for (auto &r : runs_)
        for (const BamRecInfo &x : r.second.info) keys[at++] = x.key;
#ifndef GWA_BAM_SORT_HOST_ONLY
      if (device_ >= 0) bamSortOrderDevice(device_, keys.data(), N, perm.data());
      else
#endif
        orderHost(keys.data(), N, perm.data());
    }
    st_.order_s += now() - t;
    // the duplicate templates: one bit per global template ordinal (run-major input ordinal of the leader)
    std::vector<uint32_t> dupBits;
    if (markdup_) {
      t = now();
      std::vector<BamDupInfo> all(N);
      uint64_t at = 0;
      size_t k = 0;
      for (auto &r : runs_) {
        for (BamDupInfo x : r.second.dup) {
          x.leader = (uint32_t)(runStart[k] + x.leader);
          all[at++] = x;
        }
        ds.templates += r.second.templates;
        ++k;
      }
      dupBits.assign((size_t)((N + 31) / 32), 0u);
#ifndef GWA_BAM_SORT_HOST_ONLY
      if (device_ >= 0) bamDupResolveDevice(device_, all.data(), N, N, dupBits.data(), &ds);
      else
#endif
        bamdup::resolveHost(all.data(), N, N, dupBits, &ds);
      ds.resolve_s = now() - t;
      ds.keys_s = dupKeysS_;
    }
    // 2.-5. the copy into parts of whole slices, each compressed and written
    const uint64_t partBytes = (uint64_t)partSlices_ * kSlice;
    std::vector<uint8_t> part(N ? partBytes : 0), blocks, rec;
    std::vector<uint64_t> blockStart;
    uint64_t fill = 0, filePos = (uint64_t)H;
    auto flush = [&]() {
      if (!fill) return;
      double t1 = now();
      compressPart(device_, part.data(), fill, blocks);
      st_.compress_s += now() - t1;
      uint64_t p = 0;
      while (p < blocks.size()) {
        if (blocks.size() - p < 18) throw std::runtime_error("gwa_bam_sorter: a truncated BGZF block");
        blockStart.push_back(filePos + p);
        p += (uint64_t)ld16(blocks.data() + p + 16) + 1;
      }
      if (p != blocks.size()) throw std::runtime_error("gwa_bam_sorter: the BGZF blocks do not end at the buffer's end");
      t1 = now();
      writeAll(fdBam, blocks.data(), blocks.size(), "the BAM blocks");
      st_.write_s += now() - t1;
      filePos += blocks.size();
      st_.out_bytes += blocks.size();
      fill = 0;
    };
    t = now();
    for (uint64_t i = 0; i < N; ++i) {
      const uint64_t gidx = perm[i];
      const size_t k = (size_t)(std::upper_bound(runStart.begin(), runStart.end(), gidx) - runStart.begin()) - 1;
      Cursor &c = cur[k];
      Run &run = *c.run;
      if (gidx - runStart[k] != c.next) throw std::runtime_error("gwa_bam_sorter: a run is not in key order");
      const uint32_t size = run.info[c.next].size;
      if (c.off + size > run.len) throw std::runtime_error("gwa_bam_sorter: a run is shorter than its records");
      uint8_t *src;
      if (run.path.empty()) {
        src = run.bytes.data() + c.off;
      } else {
        if (!c.f) {
          c.f = fopen(run.path.c_str(), "rb");
          if (!c.f) throw std::runtime_error("gwa_bam_sorter: cannot reopen " + run.path + ": " + strerror(errno));
        }
        rec.resize(size);
        if (fread(rec.data(), 1, size, c.f) != size) throw std::runtime_error("gwa_bam_sorter: reading back " + run.path + " failed");
        src = rec.data();
      }
      if (markdup_) {  // (before the copy: a record straddling two parts needs no special case)
        const BamDupInfo &d = run.dup[c.next];
        const uint64_t o = runStart[k] + d.leader;
        if (d.endKey != bamdup::kNoKey && (dupBits[o >> 5] >> (o & 31) & 1u)) {
          src[bamdup::kFlagByte] |= (uint8_t)(bamdup::kDupFlag >> 8);
          ++ds.dup_records;
        }
      }
      uint32_t done = 0;
      while (done < size) {
        const uint64_t take = std::min<uint64_t>(size - done, partBytes - fill);
        memcpy(part.data() + fill, src + done, take);
        fill += take;
        done += (uint32_t)take;
        if (fill == partBytes) {
          st_.copy_s += now() - t;
          flush();
          t = now();
        }
      }
      c.off += size;
      if (++c.next == run.info.size()) {  // consumed: its bytes are no longer needed
        if (c.f) {
          fclose(c.f);
          c.f = nullptr;
        }
        if (!run.path.empty()) {
          (void)unlink(run.path.c_str());
          run.path.clear();
        }
        std::vector<uint8_t>().swap(run.bytes);
      }
    }
    st_.copy_s += now() - t;
    flush();
    blockStart.push_back(filePos);
    st_.blocks = blockStart.size() - 1;
    // 6.-7. the index
    if (fdBai >= 0) {
      t = now();
      BaiWriter w(lengths_.size(), blockStart);
      for (uint64_t i = 0; i < N; ++i) {
        const size_t k = (size_t)(std::upper_bound(runStart.begin(), runStart.end(), (uint64_t)perm[i]) - runStart.begin()) - 1;
        w.add(cur[k].run->info[perm[i] - runStart[k]]);
      }
      std::vector<uint8_t> bai;
      w.write(bai);
      writeAll(fdBai, bai.data(), bai.size(), "the index");
      st_.bai_bytes = bai.size();
      st_.index_s += now() - t;
    }
  } catch (...) {
    closeAll();
    dropRuns();
    added_ = false;
    dupKeysS_ = 0;
    throw;
  }
  closeAll();
  dropRuns();
  if (stOut) *stOut = st_;
  st_ = BamSorterStats{};
  lastDup_ = ds;
  added_ = false;
  dupKeysS_ = 0;
}

}  // namespace gwa
