// Native scheduler and KV-page allocator of the dstack_amd serving engine (continuous batching).
//
// The reference orchestrator has no serving engine: its services run vLLM/TGI containers
// (reference examples/deployment/{vllm,tgi}, docs/blog/posts/amd-mi300x-inference-benchmark.md).
// This is the MI355X-native engine's host-side runtime, in C++ so the per-step planning
// (page allocation, admission, preemption, block-table packing) never shows up next to a
// 10-30 ms decode step, even at hundreds of sequences.
//
// Model: every sequence owns a list of fixed-size KV pages (PAGE tokens each, see
// ops/csrc/paged_attn.hip).  A step is either a PREFILL step (the prompts of newly admitted
// sequences, plus recomputation of preempted ones) or a DECODE step (one new token for every
// running sequence).  Preemption = recompute: when a running sequence needs a new page and none
// is free, the most recently admitted sequence releases its pages and goes back to the head of
// the waiting queue with all its tokens as its new prompt (tokens stay with the caller).
//
// Automatic prefix caching (enable_prefix_caching, off by default): the scheduler also keeps every
// sequence's token ids, and a FULL page whose K/V are all written becomes reusable.  A page is
// identified by a chained hash of its parent page's hash and its own PAGE token ids; a hit is
// confirmed by comparing the stored ids and the parent page (id and registration generation), so a
// hash collision never hands out someone else's KV.  Pages carry reference counts; a registered
// page whose count drops to zero keeps its hash entry on an LRU list of cached-free pages (a
// sequence's pages are pushed tail first: leaves are evicted before their parents) and is evicted
// only when the free list is empty.  Admission takes the hits of the prompt's full pages, always
// leaving at least one token to compute; the plan's starts[i] = PAGE * hits, and the sequence's
// first own slot is on a fresh page, so a shared page is never written.
//
// A sequence may carry a salt (add(..., salt), default 0): it seeds the sequence's hash chain, is
// stored on every page the sequence registers and is compared on a hit, so sequences with
// different salts never share pages even for equal tokens (the engine passes the LoRA adapter
// slot + 1: the K/V of a prompt depend on the adapter that computed them).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <list>
#include <stdexcept>
#include <unordered_map>
#include <vector>

namespace py = pybind11;

namespace {

struct Seq {
  int64_t id = 0;
  int num_tokens = 0;    // prompt + generated so far
  int num_cached = 0;    // tokens whose K/V are in the cache
  int max_tokens = 0;    // cap on num_tokens (prompt + max new tokens)
  int64_t admitted = -1;  // admission order (for preemption: newest first)
  bool running = false;
  std::vector<int32_t> pages;
  // prefix caching
  std::vector<int32_t> ids;  // token ids (prompt + appended), when the caller passes them
  int start = 0;             // tokens taken from the cache at admission (a page multiple)
  int chained = 0;           // leading pages that are hits or registered: the next page to register
  uint64_t chain_hash = 0;   // hash of page chained - 1
  bool chain_open = true;    // false once a page of this sequence could not be registered
  int spec_pages = 0;        // trailing pages taken for lookahead slots (speculative decoding)
  uint64_t salt = 0;         // seeds the hash chain; pages are shared only among equal salts
};

// per-page state of the prefix cache
struct PageInfo {
  int ref = 0;
  bool registered = false;
  bool in_lru = false;
  uint64_t hash = 0;
  uint32_t gen = 0;          // bumped by every registration: a stale child never matches its parent
  int32_t parent = -1;
  uint32_t parent_gen = 0;
  uint64_t salt = 0;         // of the sequence that registered the page
  std::vector<int32_t> ids;  // the page's token ids while registered
  std::list<int32_t>::iterator lru_it;
};

constexpr uint64_t HASH_SEED = 0x9e3779b97f4a7c15ULL;

int round_up(int x, int m) { return (x + m - 1) / m * m; }

class Scheduler {
 public:
  Scheduler(int num_pages, int page_size, int max_batch, int max_prefill_tokens, int max_model_len, int pad_to,
            bool enable_prefix_caching)
      : caching_(enable_prefix_caching),
        page_size_(page_size),
        max_batch_(max_batch),
        max_prefill_tokens_(max_prefill_tokens),
        max_model_len_(max_model_len),
        pad_to_(pad_to) {
    if (num_pages <= 0 || page_size <= 0 || max_batch <= 0 || max_prefill_tokens <= 0 || pad_to <= 0)
      throw std::invalid_argument("scheduler: sizes must be positive");
    free_.reserve(num_pages);
    for (int p = num_pages - 1; p >= 0; --p) free_.push_back(p);
    num_pages_ = num_pages;
    table_width_ = (max_model_len + page_size - 1) / page_size;
    if (caching_) info_.resize(num_pages);
  }

  void add(int64_t id, int prompt_len, int max_tokens, const py::object& token_ids, uint64_t salt) {
    if (seqs_.count(id)) throw std::invalid_argument("scheduler: duplicate sequence id");
    if (prompt_len <= 0) throw std::invalid_argument("scheduler: empty prompt");
    if (prompt_len >= max_model_len_) throw std::invalid_argument("scheduler: prompt longer than max_model_len");
    if (pages_for(prompt_len + 1) > num_pages_)
      throw std::invalid_argument("scheduler: prompt does not fit in the KV cache");
    Seq s;
    s.id = id;
    s.num_tokens = prompt_len;
    s.max_tokens = std::min(max_tokens, max_model_len_);
    s.salt = salt;
    s.chain_hash = salt;
    if (!token_ids.is_none()) {
      auto arr = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(token_ids);
      if (!arr || arr.ndim() != 1 || arr.shape(0) != prompt_len)
        throw std::invalid_argument("scheduler: token_ids must be an int32 array of prompt_len entries");
      if (caching_) s.ids.assign(arr.data(), arr.data() + prompt_len);
    }
    seqs_[id] = std::move(s);
    waiting_.push_back(id);
  }

  // one more token was sampled for `id` (its K/V get written by the next decode step)
  // (`token`: its id, for the prefix cache; -1 = not given)
  void append(int64_t id, int64_t token) {
    Seq& s = get(id);
    if (caching_ && token >= 0 && (int)s.ids.size() == s.num_tokens) s.ids.push_back((int32_t)token);
    s.num_tokens += 1;
  }

  // after a step: the K/V of every token but the newest are cached
  void mark_computed(int64_t id) {
    Seq& s = get(id);
    s.num_cached = s.num_tokens;
    if (caching_) register_full_pages(s);
  }

  void finish(int64_t id) {
    auto it = seqs_.find(id);
    if (it == seqs_.end()) return;
    release(it->second);
    waiting_.erase(std::remove(waiting_.begin(), waiting_.end(), id), waiting_.end());
    running_.erase(std::remove(running_.begin(), running_.end(), id), running_.end());
    seqs_.erase(it);
  }

  bool is_done(int64_t id) const {
    auto it = seqs_.find(id);
    return it == seqs_.end() || it->second.num_tokens >= it->second.max_tokens;
  }

  // Plan the next step.  Returns a dict with
  //   kind: "prefill" | "decode" | "idle"
  //   seq_ids [n], preempted [k]
  //   prefill: starts [n] (first token to compute: 0, or the cached prefix's length with prefix
  //            caching), lens [n] (tokens to compute), offsets [n] (row of each sequence in the
  //            padded token buffer), rows (total padded rows), positions [rows], slots [rows] (-1 on
  //            padding rows); with prefix caching also block_tables [n, width] and ctx_lens [n]
  //   decode:  positions [n], slots [n], ctx_lens [n], block_tables [n, width]
  // lookahead = K > 0 (speculative decoding): a decode plan also grants every sequence up to K
  // token slots after its mandatory one, for draft tokens -- as many as stay below its token cap
  // and fit in its own pages plus the pages that are FREE once every running sequence has its
  // mandatory page (never an evicted or a preempted one).  positions and slots are then [n, K + 1]
  // (slot -1, position 0 beyond the grant), with lookahead [n] the grants; ctx_lens counts no
  // draft.  A page taken for a grant and not needed by the tokens the step kept goes back to the
  // free list at the next call, before anything is planned: speculation never causes a preemption
  // or an eviction.
  py::dict schedule(bool prefer_decode, int lookahead) {
    if (lookahead < 0) throw std::invalid_argument("scheduler: lookahead must be >= 0");
    py::dict out;
    std::vector<int64_t> preempted;
    for (auto id : running_) return_lookahead_pages(get(id));
    // admission of waiting sequences (prefill-first unless the caller asks to run decodes)
    const bool can_admit = !waiting_.empty() && (int)running_.size() < max_batch_;
    if (can_admit && !(prefer_decode && !running_.empty())) {
      std::vector<int64_t> ids;
      int rows = 0;
      while (!waiting_.empty() && (int)(running_.size() + ids.size()) < max_batch_) {
        Seq& s = get(waiting_.front());
        // prefix caching: the registered pages that match the prompt's full pages (none otherwise)
        int idle_hits = 0;  // hits that sit on the cached-free list: taking them uses up free pages
        const std::vector<int32_t> hits = caching_ ? lookup(s, idle_hits) : std::vector<int32_t>{};
        const int start = (int)hits.size() * page_size_;
        const int need = pages_for(s.num_tokens + 1) - (int)s.pages.size() - (int)hits.size();
        const int padded = round_up(s.num_tokens - start, pad_to_);
        if (!ids.empty() && rows + padded > max_prefill_tokens_) break;
        if (need > free_pages() - idle_hits) break;
        if (caching_) take_hits(s, hits);
        grow(s, s.num_tokens + 1);
        s.num_cached = start;
        s.start = start;
        s.running = true;
        s.admitted = admit_counter_++;
        ids.push_back(s.id);
        rows += padded;
        waiting_.pop_front();
      }
      if (!ids.empty()) {
        for (auto id : ids) running_.push_back(id);
        const int n = (int)ids.size();
        py::array_t<int32_t> starts(n), lens(n), offsets(n), positions(rows), slots(rows);
        auto st = starts.mutable_unchecked<1>();
        auto ln = lens.mutable_unchecked<1>();
        auto of = offsets.mutable_unchecked<1>();
        auto ps = positions.mutable_unchecked<1>();
        auto sl = slots.mutable_unchecked<1>();
        int row = 0;
        for (int i = 0; i < n; ++i) {
          const Seq& s = get(ids[i]);
          const int len = s.num_tokens - s.start;
          st(i) = s.start;
          ln(i) = len;
          of(i) = row;
          const int padded = round_up(len, pad_to_);
          for (int t = 0; t < padded; ++t) {
            ps(row + t) = t < len ? s.start + t : 0;
            sl(row + t) = t < len ? slot_of(s, s.start + t) : -1;
          }
          row += padded;
        }
        if (caching_) {
          py::array_t<int32_t> ctx(n);
          py::array_t<int32_t> tables({n, table_width_});
          auto cx = ctx.mutable_unchecked<1>();
          auto tb = tables.mutable_unchecked<2>();
          for (int i = 0; i < n; ++i) {
            const Seq& s = get(ids[i]);
            cx(i) = s.num_tokens;
            const int np = (int)s.pages.size();
            for (int j = 0; j < table_width_; ++j) tb(i, j) = j < np ? s.pages[j] : 0;
          }
          out["block_tables"] = tables;
          out["ctx_lens"] = ctx;
        }
        out["kind"] = "prefill";
        out["seq_ids"] = ids;
        out["starts"] = starts;
        out["lens"] = lens;
        out["offsets"] = offsets;
        out["rows"] = rows;
        out["positions"] = positions;
        out["slots"] = slots;
        out["preempted"] = preempted;
        return out;
      }
    }
    if (running_.empty()) {
      out["kind"] = "idle";
      out["seq_ids"] = std::vector<int64_t>{};
      out["preempted"] = preempted;
      return out;
    }
    // decode: every running sequence computes its newest token (position num_tokens - 1)
    // running_ is in admission order, so the newest sequence (the preemption victim) is always
    // at or after the one being grown: removing it never shifts the entries already handled
    size_t i = 0;
    while (i < running_.size()) {
      Seq& s = get(running_[i]);
      bool self_preempted = false;
      while (pages_for(s.num_tokens) > (int)s.pages.size() && free_pages() == 0) {
        const int64_t victim = running_.back();
        preempt(victim, preempted);
        if (victim == s.id) {
          self_preempted = true;
          break;
        }
      }
      if (self_preempted) continue;
      grow(s, s.num_tokens);
      ++i;
    }
    const int n = (int)running_.size();
    if (n == 0) {
      out["kind"] = "idle";
      out["seq_ids"] = std::vector<int64_t>{};
      out["preempted"] = preempted;
      return out;
    }
    py::array_t<int32_t> ctx(n);
    py::array_t<int32_t> tables({n, table_width_});
    auto cx = ctx.mutable_unchecked<1>();
    auto tb = tables.mutable_unchecked<2>();
    if (lookahead > 0) {
      const int K1 = lookahead + 1;
      py::array_t<int32_t> grants(n);
      py::array_t<int32_t> positions({n, K1}), slots({n, K1});
      auto gr = grants.mutable_unchecked<1>();
      auto ps = positions.mutable_unchecked<2>();
      auto sl = slots.mutable_unchecked<2>();
      for (int i = 0; i < n; ++i) {
        Seq& s = get(running_[i]);
        // the step emits at most grant + 1 tokens: they must fit under the cap
        int grant = std::max(0, std::min(lookahead, s.max_tokens - s.num_tokens - 1));
        const int room = ((int)s.pages.size() + (int)free_.size()) * page_size_ - s.num_tokens;
        grant = std::min(grant, std::max(0, room));
        const int before = (int)s.pages.size();
        grow(s, s.num_tokens + grant);  // (from free_ only: room counted no cached page)
        s.spec_pages = (int)s.pages.size() - before;
        gr(i) = grant;
        for (int j = 0; j < K1; ++j) {
          ps(i, j) = j <= grant ? s.num_tokens - 1 + j : 0;
          sl(i, j) = j <= grant ? slot_of(s, s.num_tokens - 1 + j) : -1;
        }
      }
      out["lookahead"] = grants;
      out["positions"] = positions;
      out["slots"] = slots;
    } else {
      py::array_t<int32_t> positions(n), slots(n);
      auto ps = positions.mutable_unchecked<1>();
      auto sl = slots.mutable_unchecked<1>();
      for (int i = 0; i < n; ++i) {
        const Seq& s = get(running_[i]);
        ps(i) = s.num_tokens - 1;
        sl(i) = slot_of(s, s.num_tokens - 1);
      }
      out["positions"] = positions;
      out["slots"] = slots;
    }
    for (int i = 0; i < n; ++i) {
      const Seq& s = get(running_[i]);
      cx(i) = s.num_tokens;
      const int np = (int)s.pages.size();
      for (int j = 0; j < table_width_; ++j) tb(i, j) = j < np ? s.pages[j] : 0;
    }
    out["kind"] = "decode";
    out["seq_ids"] = running_;
    out["ctx_lens"] = ctx;
    out["block_tables"] = tables;
    out["preempted"] = preempted;
    return out;
  }

  // free + cached-free (evictable) pages: what admission and preemption count on
  int free_pages() const { return (int)(free_.size() + lru_.size()); }
  int cached_pages() const { return (int)by_hash_.size(); }
  int64_t prefix_hit_tokens() const { return hit_tokens_; }
  int64_t prefix_query_tokens() const { return query_tokens_; }
  bool prefix_caching() const { return caching_; }
  // test hook: AND every page hash with `mask` (0: all pages collide), to exercise the id check
  void test_set_hash_mask(uint64_t mask) { hash_mask_ = mask; }
  int num_pages() const { return num_pages_; }
  int num_waiting() const { return (int)waiting_.size(); }
  int num_running() const { return (int)running_.size(); }
  int table_width() const { return table_width_; }
  int page_size() const { return page_size_; }
  std::vector<int32_t> pages(int64_t id) { return get(id).pages; }
  int num_tokens(int64_t id) { return get(id).num_tokens; }

 private:
  Seq& get(int64_t id) {
    auto it = seqs_.find(id);
    if (it == seqs_.end()) throw std::out_of_range("scheduler: unknown sequence id");
    return it->second;
  }
  const Seq& get(int64_t id) const {
    auto it = seqs_.find(id);
    if (it == seqs_.end()) throw std::out_of_range("scheduler: unknown sequence id");
    return it->second;
  }
  int pages_for(int tokens) const { return (tokens + page_size_ - 1) / page_size_; }
  int32_t slot_of(const Seq& s, int t) const { return s.pages[t / page_size_] * page_size_ + t % page_size_; }

  void grow(Seq& s, int tokens) {
    const int need = pages_for(tokens);
    while ((int)s.pages.size() < need) {
      if (free_.empty() && lru_.empty()) throw std::runtime_error("scheduler: out of KV pages");
      if (free_.empty()) evict_lru();
      const int32_t p = free_.back();
      s.pages.push_back(p);
      free_.pop_back();
      if (caching_) info_[p].ref = 1;
    }
  }
  // the lookahead pages of the last plan that the tokens kept since do not reach
  void return_lookahead_pages(Seq& s) {
    for (; s.spec_pages > 0 && (int)s.pages.size() > pages_for(s.num_tokens); --s.spec_pages) {
      const int32_t p = s.pages.back();  // (beyond num_cached: never registered)
      s.pages.pop_back();
      if (caching_) info_[p].ref = 0;
      free_.push_back(p);
    }
    s.spec_pages = 0;
  }
  void release(Seq& s) {
    s.spec_pages = 0;
    if (!caching_) {
      for (auto p : s.pages) free_.push_back(p);
    } else {
      // tail first: a leaf reaches the LRU list's head before its parents and is evicted first
      for (auto it = s.pages.rbegin(); it != s.pages.rend(); ++it) {
        PageInfo& pi = info_[*it];
        if (--pi.ref > 0) continue;
        if (pi.registered) {
          pi.lru_it = lru_.insert(lru_.end(), *it);
          pi.in_lru = true;
        } else {
          free_.push_back(*it);
        }
      }
      s.start = s.chained = 0;
      s.chain_hash = s.salt;
      s.chain_open = true;
    }
    s.pages.clear();
  }

  // ---- prefix cache ---------------------------------------------------------------------------
  uint64_t page_hash(uint64_t parent_hash, const int32_t* ids) const {
    uint64_t h = parent_hash ^ HASH_SEED;
    for (int i = 0; i < page_size_; ++i) {  // splitmix64 finaliser over (h, id)
      uint64_t z = h + 0x9e3779b97f4a7c15ULL + (uint64_t)(uint32_t)ids[i];
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
      h = z ^ (z >> 31);
    }
    return h & hash_mask_;
  }
  // the registered page with this hash whose ids, parent and salt are exactly these, or -1
  int32_t find_page(uint64_t h, const int32_t* ids, int32_t parent, uint64_t salt) const {
    auto range = by_hash_.equal_range(h);
    for (auto it = range.first; it != range.second; ++it) {
      const PageInfo& pi = info_[it->second];
      if (pi.salt != salt || pi.parent != parent || (parent >= 0 && pi.parent_gen != info_[parent].gen)) continue;
      if (std::equal(pi.ids.begin(), pi.ids.end(), ids)) return it->second;
    }
    return -1;
  }
  // walk the prompt's full pages through the hash map; at least one token stays to be computed
  std::vector<int32_t> lookup(const Seq& s, int& idle_hits) const {
    std::vector<int32_t> hits;
    idle_hits = 0;
    if ((int)s.ids.size() < s.num_tokens) return hits;
    const int cap = (s.num_tokens - 1) / page_size_;
    uint64_t h = s.salt;
    int32_t parent = -1;
    for (int j = 0; j < cap; ++j) {
      const int32_t* ids = s.ids.data() + (size_t)j * page_size_;
      h = page_hash(h, ids);
      const int32_t p = find_page(h, ids, parent, s.salt);
      if (p < 0) break;
      hits.push_back(p);
      if (info_[p].ref == 0) ++idle_hits;
      parent = p;
    }
    return hits;
  }
  void take_hits(Seq& s, const std::vector<int32_t>& hits) {
    for (auto p : hits) {
      PageInfo& pi = info_[p];
      if (pi.in_lru) {
        lru_.erase(pi.lru_it);
        pi.in_lru = false;
      }
      pi.ref += 1;
      s.pages.push_back(p);
    }
    s.chained = (int)hits.size();
    s.chain_hash = hits.empty() ? s.salt : info_[hits.back()].hash;
    s.chain_open = true;
    query_tokens_ += s.num_tokens;
    hit_tokens_ += (int64_t)hits.size() * page_size_;
  }
  // every page of `s` whose PAGE tokens' K/V are written becomes reusable (first registration of a
  // content wins: an identical page computed by another sequence in the same step stays private,
  // and with it the rest of that sequence's chain)
  void register_full_pages(Seq& s) {
    if (!s.running) return;
    const int full = std::min(s.num_cached, (int)s.ids.size()) / page_size_;
    while (s.chain_open && s.chained < full && s.chained < (int)s.pages.size()) {
      const int j = s.chained;
      const int32_t* ids = s.ids.data() + (size_t)j * page_size_;
      const int32_t parent = j > 0 ? s.pages[j - 1] : -1;
      const uint64_t h = page_hash(s.chain_hash, ids);
      if (find_page(h, ids, parent, s.salt) >= 0) {
        s.chain_open = false;
        break;
      }
      PageInfo& pi = info_[s.pages[j]];
      pi.registered = true;
      pi.hash = h;
      pi.gen += 1;
      pi.parent = parent;
      pi.parent_gen = parent >= 0 ? info_[parent].gen : 0;
      pi.salt = s.salt;
      pi.ids.assign(ids, ids + page_size_);
      by_hash_.emplace(h, s.pages[j]);
      s.chain_hash = h;
      s.chained = j + 1;
    }
  }
  // the least recently released cached page loses its hash entry and becomes a free page
  void evict_lru() {
    const int32_t p = lru_.front();
    lru_.pop_front();
    PageInfo& pi = info_[p];
    pi.in_lru = false;
    auto range = by_hash_.equal_range(pi.hash);
    for (auto it = range.first; it != range.second; ++it)
      if (it->second == p) {
        by_hash_.erase(it);
        break;
      }
    pi.registered = false;
    pi.ids.clear();
    free_.push_back(p);
  }
  void preempt(int64_t id, std::vector<int64_t>& preempted) {
    Seq& s = get(id);
    release(s);
    s.running = false;
    s.num_cached = 0;
    running_.erase(std::remove(running_.begin(), running_.end(), id), running_.end());
    waiting_.push_front(id);
    preempted.push_back(id);
  }

  bool caching_ = false;
  std::vector<PageInfo> info_;                          // per page (prefix caching only)
  std::unordered_multimap<uint64_t, int32_t> by_hash_;  // registered pages
  std::list<int32_t> lru_;                              // cached-free pages, least recently released first
  int64_t hit_tokens_ = 0, query_tokens_ = 0;
  uint64_t hash_mask_ = ~0ULL;
  int page_size_, max_batch_, max_prefill_tokens_, max_model_len_, pad_to_;
  int num_pages_ = 0, table_width_ = 0;
  int64_t admit_counter_ = 0;
  std::vector<int32_t> free_;
  std::unordered_map<int64_t, Seq> seqs_;
  std::deque<int64_t> waiting_;
  std::vector<int64_t> running_;
};

// N-gram ("prompt lookup") proposal for speculative decoding: for n = n_max .. n_min, the most
// recent earlier occurrence of the last n tokens of `ids` (starting at s <= len - n - 1); on the
// first n that matches, the k tokens that followed it.  The copy may run over the end of the history
// into the drafts already produced (a loop of period p therefore yields k drafts).  No match: empty.
py::array_t<int32_t> ngram_propose(const py::array_t<int32_t, py::array::c_style | py::array::forcecast>& ids, int k,
                                   int n_max, int n_min) {
  if (ids.ndim() != 1) throw std::invalid_argument("ngram_propose: ids must be one-dimensional");
  if (k < 0 || n_min < 1 || n_max < n_min) throw std::invalid_argument("ngram_propose: need k >= 0, 1 <= n_min <= n_max");
  const int32_t* x = ids.data();
  const long len = (long)ids.shape(0);
  for (long n = n_max; n >= n_min && k > 0; --n) {
    if (len < n + 1) continue;
    const int32_t* suffix = x + len - n;
    for (long s = len - n - 1; s >= 0; --s) {
      if (!std::equal(suffix, suffix + n, x + s)) continue;
      py::array_t<int32_t> out(k);
      int32_t* d = out.mutable_data();
      for (long i = 0; i < k; ++i) {
        const long src = s + n + i;
        d[i] = src < len ? x[src] : d[src - len];
      }
      return out;
    }
  }
  return py::array_t<int32_t>(0);
}

}  // namespace

PYBIND11_MODULE(_sched, m) {
  m.doc() = "dstack_amd serving: native continuous-batching scheduler and KV-page allocator";
  py::class_<Scheduler>(m, "Scheduler")
      .def(py::init<int, int, int, int, int, int, bool>(), py::arg("num_pages"), py::arg("page_size"),
           py::arg("max_batch"), py::arg("max_prefill_tokens"), py::arg("max_model_len"), py::arg("pad_to") = 128,
           py::arg("enable_prefix_caching") = false)
      .def("add", &Scheduler::add, py::arg("seq_id"), py::arg("prompt_len"), py::arg("max_tokens"),
           py::arg("token_ids") = py::none(), py::arg("salt") = (uint64_t)0)
      .def("append", &Scheduler::append, py::arg("seq_id"), py::arg("token") = -1)
      .def("_test_set_hash_mask", &Scheduler::test_set_hash_mask)
      .def("mark_computed", &Scheduler::mark_computed)
      .def("finish", &Scheduler::finish)
      .def("is_done", &Scheduler::is_done)
      .def("schedule", &Scheduler::schedule, py::arg("prefer_decode") = false, py::arg("lookahead") = 0)
      .def("pages", &Scheduler::pages)
      .def("num_tokens", &Scheduler::num_tokens)
      .def_property_readonly("free_pages", &Scheduler::free_pages)
      .def_property_readonly("cached_pages", &Scheduler::cached_pages)
      .def_property_readonly("prefix_hit_tokens", &Scheduler::prefix_hit_tokens)
      .def_property_readonly("prefix_query_tokens", &Scheduler::prefix_query_tokens)
      .def_property_readonly("enable_prefix_caching", &Scheduler::prefix_caching)
      .def_property_readonly("num_pages", &Scheduler::num_pages)
      .def_property_readonly("num_waiting", &Scheduler::num_waiting)
      .def_property_readonly("num_running", &Scheduler::num_running)
      .def_property_readonly("table_width", &Scheduler::table_width)
      .def_property_readonly("page_size", &Scheduler::page_size);
  m.def("ngram_propose", &ngram_propose, py::arg("ids"), py::arg("k"), py::arg("n_max") = 3, py::arg("n_min") = 1);
}
