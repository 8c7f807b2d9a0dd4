// bam_sorter.h -- the run sorter behind gwa_bam_sorter_* (include/gwa.h "Sorted BAM"): sorted runs, one per
// batch, held in host memory or spilled to files, and finish(): the global order, the copy into parts of whole
// BGZF slices, their compression, and the .bai.  Compiles without HIP with GWA_BAM_SORT_HOST_ONLY (the host
// test program): device must then be < 0.
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "bam_dup_core.h"
#include "bam_sort_core.h"

namespace gwa {

struct BamSorterStats {
  uint64_t records = 0, bytes = 0, runs = 0, spilled_runs = 0, spilled_bytes = 0, blocks = 0, out_bytes = 0, bai_bytes = 0;
  double add_s = 0, order_s = 0, copy_s = 0, compress_s = 0, write_s = 0, index_s = 0;
};

class BamSorter {
 public:
  // names / lengths: the contig table the records' refID indexes; tmpDir may be null (no spilling)
  BamSorter(std::vector<std::string> names, std::vector<int64_t> lengths, int device, const char *tmpDir, uint64_t memBytes);
  ~BamSorter();
  BamSorter(const BamSorter &) = delete;
  BamSorter &operator=(const BamSorter &) = delete;

  // unsorted caller bytes: validated, sorted (on the device, or by the host build for device < 0), kept as a run
  void addRecords(uint64_t runId, const uint8_t *bytes, uint64_t len);
  // a batch's sorted records and their per-record array
  void addSortedRun(uint64_t runId, std::vector<uint8_t> &&sorted, std::vector<bamsort::BamRecInfo> &&info);
  // the same with the records' duplicate-marking entries, in the same order (needed when marking is on)
  void addSortedRun(uint64_t runId, std::vector<uint8_t> &&sorted, std::vector<bamsort::BamRecInfo> &&info,
                    std::vector<bamdup::BamDupInfo> &&dup);
  // Duplicate marking (include/gwa.h "Duplicate marking") for the runs added from now on; refused once a run
  // of the current scope has been added.
  void setMarkdup(bool on);
  bool markdup() const { return markdup_; }
  // counts and times of the last finish with marking on (zero otherwise)
  bamdup::DupStats markdupStats() const { return lastDup_; }
  // seconds of a run's per-run duplicate pass made before addSortedRun: counted as keys_s
  void addDupSeconds(double s) {
    std::lock_guard<std::mutex> g(mu_);
    dupKeysS_ += s;
  }
  // the sorted stream as BGZF blocks to fdBam, the index to fdBai (-1: none); the runs are consumed
  void finish(int fdBam, int fdBai, BamSorterStats *st);
  // seconds spent on a run before addSortedRun (a batch's device sort and its copy to the host): counted as add_s
  void addSeconds(double s) {
    std::lock_guard<std::mutex> g(mu_);
    st_.add_s += s;
  }
  void setPartSlices(uint32_t slices) { partSlices_ = slices ? slices : 1; }  // (tests: a part of one slice)
  int device() const { return device_; }

 private:
  struct Run {
    std::vector<uint8_t> bytes;  // empty when spilled
    std::vector<bamsort::BamRecInfo> info;
    std::vector<bamdup::BamDupInfo> dup;  // in the same order; only with duplicate marking
    uint64_t templates = 0;
    std::string path;            // the spill file
    uint64_t len = 0;
  };
  void dropRuns();
  std::vector<std::string> names_;
  std::vector<int64_t> lengths_;
  int device_;
  bool haveTmp_;
  std::string tmpDir_;
  uint64_t memBytes_, memUsed_ = 0, serial_ = 0;
  uint32_t partSlices_ = 256;
  std::mutex mu_;
  std::map<uint64_t, Run> runs_;
  BamSorterStats st_;
  bool markdup_ = false, added_ = false;
  double dupKeysS_ = 0;
  bamdup::DupStats lastDup_;
};

}  // namespace gwa
