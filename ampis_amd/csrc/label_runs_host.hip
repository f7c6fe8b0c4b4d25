// Host side of amp_label_runs (mask_analysis.h): the argument check, the capacity report that both paths share, and the evaluation with a NULL
// context -- the instances of an annotation image (ampis/data_utils.py:412-428: label the foreground, `ann == u` per instance, encode each) as
// COCO run lists, without a dense mask per instance.  A two-pass run-based union-find:
//   pass 1  the vertical runs of every column (foreground runs of a BINARY image, constant-id runs of a LABEL image; a run never crosses a
//           column end), in column-major order -- the order of the COCO positions col * h + row;
//   union   BINARY only: the runs of column c against the runs of column c - 1 whose rows meet theirs (one row wider on each side for 8
//           neighbours), two pointers over both lists; the larger root goes under the smaller;
//   pass 2  the key of an instance -- the smallest row-major position of its runs, or its id -- and the rank of the key among the distinct keys
//           is the instance; a counting sort by rank keeps the column-major order inside an instance; box, area and counts from its runs, two
//           runs joined where one ends at the last row of a column and the next starts at the first row of the following one.
// Plain C++ throughout, integers only: the host-only sanitizer build of tests/sanitize compiles this file with g++.  label_runs.hip computes the
// same bytes on the device.
#include <algorithm>
#include <vector>

#include "common.h"
#include "mask_analysis.h"

namespace amp {

int label_runs_check(const void* image, int h, int w, int kind, int connectivity, const int* ids, const int* boxes, const unsigned int* areas,
                     const uint32_t* counts, const unsigned long long* counts_off, const int* counts_len, int inst_cap,
                     const unsigned long long* need) {
    AMP_REQUIRE(h >= 1 && w >= 1 && (unsigned long long)h * (unsigned long long)w <= (1ull << 30),
                "amp_label_runs: image size %d x %d (at least 1 a side, at most 2^30 pixels)", h, w);
    AMP_REQUIRE(kind == AMP_LABEL_BINARY || kind == AMP_LABEL_IDS, "amp_label_runs: kind = %d (0 binary, 1 label ids)", kind);
    AMP_REQUIRE(connectivity == 1 || connectivity == 2, "amp_label_runs: connectivity = %d (1: 4 neighbours, 2: 8 neighbours)", connectivity);
    AMP_REQUIRE(inst_cap >= 0, "amp_label_runs: inst_cap = %d", inst_cap);
    AMP_REQUIRE(image, "amp_label_runs: null argument image");
    AMP_REQUIRE(need, "amp_label_runs: null argument need");
    AMP_REQUIRE(ids && boxes && areas && counts && counts_off && counts_len, "amp_label_runs: null argument %s",
                !ids ? "ids" : !boxes ? "boxes" : !areas ? "areas" : !counts ? "counts" : !counts_off ? "counts_off" : "counts_len");
    return AMP_OK;
}

int label_runs_capacity(unsigned long long instances, unsigned long long counts, int inst_cap, unsigned long long counts_cap,
                        unsigned long long* need) {
    need[0] = instances;
    need[1] = counts;
    if (instances > (unsigned long long)inst_cap || counts > counts_cap) {
        set_error("amp_label_runs: inst_cap = %d, counts_cap = %llu; %llu instances and %llu counts are needed", inst_cap, counts_cap, instances,
                  counts);
        return AMP_ERR_NOMEM;
    }
    return AMP_OK;
}

int label_runs_host(const void* image, int h, int w, int kind, int connectivity, int zero_is_background, int* ids, int* boxes,
                    unsigned int* areas, uint32_t* counts, unsigned long long* counts_off, int* counts_len, int inst_cap,
                    unsigned long long counts_cap, int* labels, unsigned long long* need) {
    const uint32_t area = (uint32_t)((unsigned long long)h * w);
    std::vector<uint32_t> S, E;                   // run k = pixels [S[k], E[k]) of the column-major image, inside one column
    std::vector<int> V;                           // its id (LABEL)
    std::vector<uint32_t> colstart((size_t)w + 1, 0u);
    for (int c = 0; c < w; ++c) {
        colstart[c] = (uint32_t)S.size();
        const uint32_t cb = (uint32_t)c * (uint32_t)h;
        int r = 0;
        while (r < h) {
            const int v = label_pixel(image, kind, (size_t)r * w + c);
            int e = r + 1;
            while (e < h && label_pixel(image, kind, (size_t)e * w + c) == v) ++e;      // ends: e grows to h
            if (label_is_instance(v, kind, zero_is_background)) { S.push_back(cb + r); E.push_back(cb + e); V.push_back(v); }
            r = e;
        }
    }
    const size_t R = S.size();
    colstart[w] = (uint32_t)R;

    std::vector<uint32_t> key(R);                 // per run: the key of its instance
    if (kind == AMP_LABEL_BINARY) {
        std::vector<uint32_t> parent(R);
        for (size_t i = 0; i < R; ++i) parent[i] = (uint32_t)i;
        auto find = [&](uint32_t x) {
            while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }     // ends: parent[x] < x until the root
            return x;
        };
        const uint32_t d = connectivity == 2 ? 1u : 0u;
        for (int c = 1; c < w; ++c) {
            const uint32_t shift = (uint32_t)h;   // a run of column c - 1 moved one column right
            uint32_t j = colstart[c - 1];
            const uint32_t jend = colstart[c];
            for (uint32_t i = colstart[c]; i < colstart[c + 1]; ++i) {
                while (j < jend && E[j] + shift + d <= S[i]) ++j;                          // runs that end above run i end above every later one
                for (uint32_t k = j; k < jend && S[k] + shift < E[i] + d; ++k) {
                    uint32_t a = find(i), b = find(k);
                    if (a == b) continue;
                    if (a < b) std::swap(a, b);
                    parent[a] = b;
                }
            }
        }
        std::vector<uint32_t> first(R, 0xffffffffu);      // per root: the smallest row-major position of its runs (a run's is its top pixel's)
        for (size_t i = 0; i < R; ++i) {
            const uint32_t root = find((uint32_t)i), c = S[i] / (uint32_t)h, r = S[i] - c * (uint32_t)h;
            first[root] = std::min(first[root], r * (uint32_t)w + c);
            key[i] = root;
        }
        for (size_t i = 0; i < R; ++i) key[i] = first[key[i]];
    } else {
        for (size_t i = 0; i < R; ++i) key[i] = (uint32_t)V[i] ^ 0x80000000u;              // ascending unsigned = ascending signed
    }

    std::vector<uint32_t> distinct(key);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    const size_t N = distinct.size();
    std::vector<uint32_t> rank(R), first_run(N + 1, 0u), order(R);
    for (size_t i = 0; i < R; ++i) {
        rank[i] = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), key[i]) - distinct.begin());
        ++first_run[rank[i] + 1];
    }
    for (size_t n = 0; n < N; ++n) first_run[n + 1] += first_run[n];
    {
        std::vector<uint32_t> at(first_run.begin(), first_run.end() - 1);
        for (size_t i = 0; i < R; ++i) order[at[rank[i]]++] = (uint32_t)i;               // stable: column-major order inside an instance
    }

    std::vector<uint32_t> out;                    // the counts of all instances, back to back
    std::vector<unsigned long long> off(N);
    std::vector<int> box(4 * N);
    std::vector<uint32_t> ar(N);
    for (size_t n = 0; n < N; ++n) {
        off[n] = out.size();
        int r0 = h, r1 = 0, c0 = w, c1 = 0;
        uint32_t prev = 0, px = 0;                // the boundary before, the pixels so far
        for (uint32_t q = first_run[n]; q < first_run[n + 1]; ++q) {
            const uint32_t i = order[q], s = S[i], e = E[i];
            const int c = (int)(s / (uint32_t)h), ra = (int)(s - (uint32_t)c * (uint32_t)h), rb = (int)(e - (uint32_t)c * (uint32_t)h);
            r0 = std::min(r0, ra); r1 = std::max(r1, rb); c0 = std::min(c0, c); c1 = std::max(c1, c + 1);
            px += e - s;
            if (!(q > first_run[n] && E[order[q - 1]] == s)) { out.push_back(s - prev); prev = s; }         // joined with the run before: no boundary
            if (!(q + 1 < first_run[n + 1] && S[order[q + 1]] == e)) { out.push_back(e - prev); prev = e; }
        }
        if (prev != area) out.push_back(area - prev);
        box[4 * n] = r0; box[4 * n + 1] = c0; box[4 * n + 2] = r1; box[4 * n + 3] = c1;
        ar[n] = px;
    }

    AMP_TRY_STATUS(label_runs_capacity(N, out.size(), inst_cap, counts_cap, need));
    for (size_t n = 0; n < N; ++n) {
        ids[n] = kind == AMP_LABEL_BINARY ? (int)n + 1 : (int)(distinct[n] ^ 0x80000000u);
        areas[n] = ar[n];
        counts_off[n] = off[n];
        counts_len[n] = (int)((n + 1 < N ? off[n + 1] : (unsigned long long)out.size()) - off[n]);
    }
    std::copy(box.begin(), box.end(), boxes);
    std::copy(out.begin(), out.end(), counts);
    if (labels) {
        std::fill(labels, labels + (size_t)area, 0);
        for (size_t i = 0; i < R; ++i) {
            const uint32_t c = S[i] / (uint32_t)h, ra = S[i] - c * (uint32_t)h, rb = E[i] - c * (uint32_t)h;
            for (uint32_t r = ra; r < rb; ++r) labels[(size_t)r * w + c] = (int)rank[i] + 1;
        }
    }
    return AMP_OK;
}

}  // namespace amp
