// Host-side COCO RLE codec of the C ABI.  Replaces the pycocotools.mask calls AMPIS makes on the
// output of the hot path: encode (ampis/data_utils.py:275), decode/area (ampis/structures.py:465-468,568,752),
// iou (ampis/analyze.py:108,158), merge (ampis/analyze.py:315-321, ampis/applications/powder.py:82-83).
// pycocotools 2.0.4 (docker/env.yml:21) is not vendored in the reference; this follows its published format:
// column-major runs alternating 0/1 starting with a 0-run; the `counts` string stores each run as 5-bit groups, LSB first,
// char = group + 48, bit 0x20 = continuation, bit 0x10 of the last group = sign, runs i > 2 stored as a delta against
// run i-2.  Byte format pinned by the reference's five result pickles (tests/golden/rle_pickles.json).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "region_props.h"
#include "seg_class_map.h"

extern "C" {

int amp_rle_to_string(const uint32_t* cnts, int m, char* out, size_t cap, size_t* len) {
    AMP_REQUIRE((cnts || m == 0) && out && len && m >= 0, "amp_rle_to_string: bad argument");
    size_t p = 0;
    for (int i = 0; i < m; ++i) {
        long long x = (long long)cnts[i];
        if (i > 2) x -= (long long)cnts[i - 2];
        bool more = true;
        while (more) {
            int c = (int)(x & 0x1f);
            x >>= 5;   // arithmetic shift keeps the sign
            more = (c & 0x10) ? (x != -1) : (x != 0);
            if (more) c |= 0x20;
            AMP_REQUIRE(p + 1 < cap, "amp_rle_to_string: output buffer too small (cap=%zu)", cap);
            out[p++] = (char)(c + 48);
        }
    }
    out[p] = 0;
    *len = p;
    return AMP_OK;
}

/* n run-length lists out of one pool (list i = pool[off[i] .. off[i] + len[i])) -> n counts strings, back to back in `out`;
 * string i = out[str_off[i] .. str_off[i + 1]).  One call per image instead of one per mask (a ctypes round trip each). */
int amp_rle_to_strings(const uint32_t* pool, const unsigned long long* off, const int* len, int n, char* out, size_t cap,
                       size_t* str_off) {
    AMP_REQUIRE((pool || n == 0) && (off || n == 0) && (len || n == 0) && out && str_off && n >= 0, "amp_rle_to_strings: bad argument");
    size_t p = 0;
    str_off[0] = 0;
    for (int i = 0; i < n; ++i) {
        size_t l = 0;
        AMP_REQUIRE(p < cap, "amp_rle_to_strings: output buffer too small (cap=%zu)", cap);
        const int st = amp_rle_to_string(pool + off[i], len[i], out + p, cap - p, &l);
        if (st != AMP_OK) return st;
        p += l;
        str_off[i + 1] = p;
    }
    return AMP_OK;
}

int amp_rle_from_string(const char* s, size_t len, uint32_t* cnts, int cap, int* m_out) {
    AMP_REQUIRE((s || len == 0) && cnts && m_out, "amp_rle_from_string: null argument");
    int m = 0;
    size_t p = 0;
    while (p < len) {
        unsigned long long x = 0;
        int k = 0;
        bool more = true;
        while (more) {
            AMP_REQUIRE(p < len, "amp_rle_from_string: truncated counts string");
            const int c = (int)(unsigned char)s[p] - 48;
            AMP_REQUIRE(c >= 0 && c < 64, "amp_rle_from_string: byte 0x%02x at offset %zu is not a counts character", (unsigned)(unsigned char)s[p], p);
            // a 32-bit run (or its signed delta) needs at most 7 groups of 5 bits; hostile input must not shift past the word (UB)
            AMP_REQUIRE(k < 8, "amp_rle_from_string: a run of more than 8 groups at offset %zu", p);
            x |= (unsigned long long)(c & 0x1f) << (5 * k);
            more = (c & 0x20) != 0;
            ++p;
            ++k;
            if (!more && (c & 0x10)) x |= ~0ull << (5 * k);      // sign extension
        }
        long long v = (long long)x;
        if (m > 2) v += (long long)cnts[m - 2];
        AMP_REQUIRE(v >= 0 && v <= 0xffffffffll, "amp_rle_from_string: run %d decodes to %lld (not a 32-bit run length)", m, v);
        AMP_REQUIRE(m < cap, "amp_rle_from_string: more than cap=%d runs", cap);
        cnts[m++] = (uint32_t)v;
    }
    *m_out = m;
    return AMP_OK;
}

// mask: column-major (Fortran order) h*w bytes, non-zero = foreground.
int amp_rle_encode(const uint8_t* mask_colmajor, int h, int w, uint32_t* cnts, int cap, int* m_out) {
    AMP_REQUIRE(mask_colmajor && cnts && m_out && h >= 0 && w >= 0, "amp_rle_encode: bad argument");
    const size_t a = (size_t)h * w;
    int m = 0;
    uint32_t c = 0;
    uint8_t p = 0;
    for (size_t j = 0; j < a; ++j) {
        const uint8_t v = mask_colmajor[j] ? 1 : 0;
        if (v != p) {
            AMP_REQUIRE(m < cap, "amp_rle_encode: more than cap=%d runs", cap);
            cnts[m++] = c;
            c = 0;
            p = v;
        }
        ++c;
    }
    AMP_REQUIRE(m < cap, "amp_rle_encode: more than cap=%d runs", cap);
    cnts[m++] = c;
    *m_out = m;
    return AMP_OK;
}

int amp_rle_decode(const uint32_t* cnts, int m, int h, int w, uint8_t* mask_colmajor) {
    AMP_REQUIRE((cnts || m == 0) && mask_colmajor, "amp_rle_decode: null argument");
    const size_t a = (size_t)h * w;
    size_t pos = 0;
    uint8_t v = 0;
    for (int i = 0; i < m; ++i) {
        AMP_REQUIRE(pos + cnts[i] <= a, "amp_rle_decode: runs exceed h*w");
        std::fill(mask_colmajor + pos, mask_colmajor + pos + cnts[i], v);
        pos += cnts[i];
        v = !v;
    }
    AMP_REQUIRE(pos == a, "amp_rle_decode: runs sum to %zu, expected %zu", pos, a);
    return AMP_OK;
}

int amp_rle_area(const uint32_t* cnts, int m, unsigned long long* area) {
    AMP_REQUIRE((cnts || m == 0) && area, "amp_rle_area: null argument");
    unsigned long long s = 0;
    for (int i = 1; i < m; i += 2) s += cnts[i];
    *area = s;
    return AMP_OK;
}

}  // extern "C"

// Walk two run lists in lock step; fn(len, va, vb) for each maximal stretch where both values are constant.
template <class F>
static void rle_zip(const uint32_t* A, int ka, const uint32_t* B, int kb, F fn) {
    unsigned long long ca = ka ? A[0] : 0, cb = kb ? B[0] : 0;
    int a = 1, b = 1;
    bool va = false, vb = false;
    unsigned long long ct = 1;
    while (ct > 0) {
        const unsigned long long c = std::min(ca, cb);
        fn(c, va, vb);
        ct = 0;
        ca -= c;
        if (!ca && a < ka) { ca = A[a++]; va = !va; }
        ct += ca;
        cb -= c;
        if (!cb && b < kb) { cb = B[b++]; vb = !vb; }
        ct += cb;
    }
}

extern "C" {

// IoU of mask d (dt) against mask g (gt); iscrowd: union replaced by area(dt). Same values as pycocotools rleIou
// (0 when the intersection is empty).
int amp_rle_iou(const uint32_t* dt, int md, const uint32_t* gt, int mg, int iscrowd, double* iou) {
    AMP_REQUIRE(dt && gt && iou && md > 0 && mg > 0, "amp_rle_iou: bad argument");
    unsigned long long i = 0, u = 0;
    rle_zip(dt, md, gt, mg, [&](unsigned long long c, bool va, bool vb) {
        if (va || vb) {
            u += c;
            if (va && vb) i += c;
        }
    });
    if (i == 0) u = 1;
    else if (iscrowd) (void)amp_rle_area(dt, md, &u);
    *iou = (double)i / (double)u;
    return AMP_OK;
}

/* IoU of every pair out of two pools of run-length lists (list i = pool[off[i] .. off[i] + len[i])): out[d * ng + g], the matrix
 * pycocotools.mask.iou(dt, gt, iscrowd) returns.  Like rleIou it looks at the bounding boxes first (h = mask height, 0 = skip that
 * test): boxes that do not overlap mean IoU 0 without walking the runs -- for a few hundred instances per micrograph that is all but
 * a few pairs per row. */
int amp_rle_iou_matrix(const uint32_t* dpool, const unsigned long long* doff, const int* dlen, int nd, const uint32_t* gpool,
                       const unsigned long long* goff, const int* glen, int ng, const unsigned char* iscrowd, int h, double* out) {
    AMP_REQUIRE(nd >= 0 && ng >= 0 && h >= 0 && (nd == 0 || (dpool && doff && dlen)) && (ng == 0 || (gpool && goff && glen)) &&
                (out || nd == 0 || ng == 0), "amp_rle_iou_matrix: bad argument");
    struct Box { long long x0, x1, y0, y1; bool any; };
    auto bbox = [&](const uint32_t* c, int m) {
        Box b{1LL << 60, -1, 1LL << 60, -1, false};
        unsigned long long p = 0;
        for (int i = 0; i < m; ++i) {
            const unsigned long long l = c[i];
            if ((i & 1) && l > 0) {
                b.any = true;
                if (h > 0) {
                    const long long xa = (long long)(p / h), xb = (long long)((p + l - 1) / h);
                    b.x0 = std::min(b.x0, xa); b.x1 = std::max(b.x1, xb);
                    if (xa == xb) { b.y0 = std::min(b.y0, (long long)(p % h)); b.y1 = std::max(b.y1, (long long)((p + l - 1) % h)); }
                    else { b.y0 = 0; b.y1 = h - 1; }
                } else {
                    b.x0 = std::min(b.x0, (long long)p); b.x1 = std::max(b.x1, (long long)(p + l - 1));   // linear extent
                    b.y0 = 0; b.y1 = 0;
                }
            }
            p += l;
        }
        return b;
    };
    std::vector<Box> db((size_t)nd), gb((size_t)ng);
    for (int d = 0; d < nd; ++d) { AMP_REQUIRE(dlen[d] > 0, "amp_rle_iou_matrix: empty run list"); db[d] = bbox(dpool + doff[d], dlen[d]); }
    for (int g = 0; g < ng; ++g) { AMP_REQUIRE(glen[g] > 0, "amp_rle_iou_matrix: empty run list"); gb[g] = bbox(gpool + goff[g], glen[g]); }
    for (int d = 0; d < nd; ++d)
        for (int g = 0; g < ng; ++g) {
            const Box &a = db[d], &b = gb[g];
            double v = 0.0;
            if (a.any && b.any && a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1) {
                const int st = amp_rle_iou(dpool + doff[d], dlen[d], gpool + goff[g], glen[g], iscrowd ? (int)iscrowd[g] : 0, &v);
                if (st != AMP_OK) return st;
            }
            out[(size_t)d * ng + g] = v;
        }
    return AMP_OK;
}

// out = A & B (intersect != 0) or A | B, both over the same h*w. Returns the number of runs in *m_out.
int amp_rle_pair_overlap(const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                         const unsigned long long* boff, const int* blen, const int* pair_a, const int* pair_b, int npairs,
                         unsigned long long* inter, unsigned long long* only_a, unsigned long long* only_b) {
    AMP_REQUIRE(npairs >= 0 && (npairs == 0 || (apool && aoff && alen && bpool && boff && blen && pair_a && pair_b && inter && only_a && only_b)),
                "amp_rle_pair_overlap: bad argument");
    for (int p = 0; p < npairs; ++p) {
        const int ia = pair_a[p], ib = pair_b[p];
        AMP_REQUIRE(ia >= 0 && ib >= 0 && alen[ia] > 0 && blen[ib] > 0, "amp_rle_pair_overlap: pair %d names an empty run list", p);
        unsigned long long both = 0, a = 0, b = 0;      // one pass over the two run lists: the three pixel classes of the pair
        rle_zip(apool + aoff[ia], alen[ia], bpool + boff[ib], blen[ib], [&](unsigned long long c, bool va, bool vb) {
            if (va && vb) both += c;
            else if (va) a += c;
            else if (vb) b += c;
        });
        inter[p] = both; only_a[p] = a; only_b[p] = b;
    }
    return AMP_OK;
}

int amp_rle_merge2(const uint32_t* A, int ka, const uint32_t* B, int kb, int intersect, uint32_t* out, int cap, int* m_out) {
    AMP_REQUIRE(A && B && out && m_out && ka > 0 && kb > 0, "amp_rle_merge2: bad argument");
    int m = 0;
    bool v = false;
    unsigned long long cc = 0;
    bool overflow = false;
    unsigned long long ca = A[0], cb = B[0];
    int a = 1, b = 1;
    bool va = false, vb = false;
    unsigned long long ct = 1;
    while (ct > 0) {
        const unsigned long long c = std::min(ca, cb);
        cc += c;
        ct = 0;
        ca -= c;
        if (!ca && a < ka) { ca = A[a++]; va = !va; }
        ct += ca;
        cb -= c;
        if (!cb && b < kb) { cb = B[b++]; vb = !vb; }
        ct += cb;
        const bool vp = v;
        v = intersect ? (va && vb) : (va || vb);
        if (v != vp || ct == 0) {
            if (m < cap) out[m++] = (uint32_t)cc; else overflow = true;
            cc = 0;
        }
    }
    AMP_REQUIRE(!overflow, "amp_rle_merge2: more than cap=%d runs", cap);
    *m_out = m;
    return AMP_OK;
}

}  // extern "C"

extern "C" {

// Polygon (flat x0,y0,x1,y1,... ; k vertices) -> run lengths of an h x w mask: pycocotools maskApi.c rleFrPoly, the routine behind
// RLE.frPyObjects (ampis/structures.py:677) and detectron2's polygons_to_bitmask.  Boundary is traced on a 5x upsampled grid,
// x-crossings become run boundaries, sorted, differenced, zero-length runs merged.
int amp_rle_from_polygon(const double* xy, int k, int h, int w, uint32_t* cnts, int cap, int* m_out) {
    AMP_REQUIRE(xy && cnts && m_out && k >= 1 && h > 0 && w > 0, "amp_rle_from_polygon: bad argument");
    const double scale = 5.0;
    std::vector<int> x(k + 1), y(k + 1);
    for (int j = 0; j < k; ++j) { x[j] = (int)(scale * xy[2 * j] + 0.5); y[j] = (int)(scale * xy[2 * j + 1] + 0.5); }
    x[k] = x[0]; y[k] = y[0];
    std::vector<unsigned long long> a;
    for (int j = 0; j < k; ++j) {
        int xs = x[j], xe = x[j + 1], ys = y[j], ye = y[j + 1];
        const int dx = std::abs(xe - xs), dy = std::abs(ys - ye);
        const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
        if (flip) { std::swap(xs, xe); std::swap(ys, ye); }
        const int len = dx >= dy ? dx : dy;
        const double s = dx >= dy ? (dx ? (double)(ye - ys) / dx : 0.0) : (double)(xe - xs) / dy;
        int pu = 0, pv = 0;
        for (int d = 0; d <= len; ++d) {
            const int t = flip ? len - d : d;
            int u, v;
            if (dx >= dy) { u = t + xs; v = (int)(ys + s * t + 0.5); } else { v = t + ys; u = (int)(xs + s * t + 0.5); }
            if (d > 0 && u != pu) {   // consecutive edges share their vertex, so pairs across edges never differ
                double xd = (double)(u < pu ? u : u - 1);
                xd = (xd + 0.5) / scale - 0.5;
                if (std::floor(xd) == xd && xd >= 0 && xd <= w - 1) {
                    double yd = (double)(v < pv ? v : pv);
                    yd = (yd + 0.5) / scale - 0.5;
                    if (yd < 0) yd = 0; else if (yd > h) yd = h;
                    yd = std::ceil(yd);
                    a.push_back((unsigned long long)xd * (unsigned long long)h + (unsigned long long)yd);
                }
            }
            pu = u; pv = v;
        }
    }
    a.push_back((unsigned long long)h * (unsigned long long)w);
    std::sort(a.begin(), a.end());
    unsigned long long p = 0;
    for (auto& v : a) { const unsigned long long t = v; v -= p; p = t; }
    std::vector<unsigned long long> b;
    size_t j = 0;
    b.push_back(a[j++]);
    while (j < a.size()) {
        if (a[j] > 0) b.push_back(a[j++]);
        else { ++j; if (j < a.size()) b.back() += a[j++]; }
    }
    AMP_REQUIRE((int)b.size() <= cap, "amp_rle_from_polygon: more than cap=%d runs", cap);
    for (size_t i = 0; i < b.size(); ++i) cnts[i] = (uint32_t)b[i];
    *m_out = (int)b.size();
    return AMP_OK;
}

}  // extern "C"

// ---- nearest-neighbour resize (+ horizontal mirror) of a mask IN THE RUN-LENGTH DOMAIN -----------------------------------------------
// What detectron2 does to a bitmask annotation when the image is resized: ResizeTransform.apply_segmentation = PIL Image.resize(NEAREST)
// of the decoded mask (then HFlipTransform).  Decoding, resizing and re-encoding every instance of a micrograph costs seconds per image on
// the host (476 instances at 1024 x 1536: 2.1 s); the same result from the runs costs microseconds.  The pixel correspondence is Pillow's
// ImagingScaleAffine, restated with its double-precision ACCUMULATION (xo += a0 per step, COORD() = truncation): output column x reads source
// column xin[x], output row y reads source row yin[y]; both tables are non-decreasing, so a run boundary of a source column maps to the
// first output row whose source row reaches it.  A crop (CropTransform before the resize: mask[y0:y0+ch, x0:x0+cw]) only shifts the two tables;
// the up-down mirror (VFlipTransform) emits a column's stretches in reverse order.
static int rle_window_resize(const char* who, const uint32_t* cnts, int m, int h, int w, int y0, int x0, int ch, int cw, int nh, int nw, int flip,
                             uint32_t* out, int cap, int* m_out) {
    auto table = [](int n_in, int n_out, int first_in, std::vector<int>& tab) {
        tab.resize((size_t)n_out);
        const double a = (double)n_in / (double)n_out;
        double o = a * 0.5;
        for (int i = 0; i < n_out; ++i) {
            int v = o < 0.0 ? -1 : (int)o;
            tab[(size_t)i] = first_in + (v < n_in ? v : n_in - 1);   // (Pillow skips coordinates beyond the image; they cannot occur for a pure scale)
            o += a;
        }
    };
    std::vector<int> xin, yin;
    table(cw, nw, x0, xin);
    table(ch, nh, y0, yin);
    // first output row that reads source row >= r, for r in [0, h]
    std::vector<int> first((size_t)h + 1);
    {
        int y = 0;
        for (int r = 0; r <= h; ++r) {
            while (y < nh && yin[(size_t)y] < r) ++y;
            first[(size_t)r] = y;
        }
    }
    // per source column: value at row 0 and the rows where the value changes (a zero-length run gives two changes at one row: they cancel)
    std::vector<int> col_start((size_t)w + 1, 0);
    std::vector<int> trans;          // transition rows, column after column
    std::vector<unsigned char> col_v0((size_t)w, 0);
    {
        unsigned long long total = 0;
        for (int j = 0; j < m; ++j) total += cnts[j];
        AMP_REQUIRE(total == (unsigned long long)h * w, "%s: the runs cover %llu pixels, the mask has %d x %d", who, total, h, w);
        int j = 0;
        unsigned long long run_end = cnts[0];
        unsigned char v = 0;
        for (int c = 0; c < w; ++c) {
            const unsigned long long top = (unsigned long long)c * h, bot = top + h;
            while (run_end <= top) { ++j; run_end += cnts[j]; v ^= 1; }
            col_v0[(size_t)c] = v;
            col_start[(size_t)c] = (int)trans.size();
            while (run_end < bot) { trans.push_back((int)(run_end - top)); ++j; run_end += cnts[j]; v ^= 1; }
        }
        col_start[(size_t)w] = (int)trans.size();
    }
    // emit the output runs column by column
    int mo = 0;
    unsigned long long run = 0;
    unsigned char cur = 0;           // COCO RLE starts with a run of zeros
    auto put = [&](unsigned char v, unsigned long long n) -> bool {
        if (n == 0) return true;
        if (v == cur) { run += n; return true; }
        if (mo >= cap) return false;
        out[mo++] = (uint32_t)run;
        cur = v; run = n;
        return true;
    };
    std::vector<int> seg;            // up-down mirror: the lengths of one column's stretches, to be emitted last to first
    for (int ox = 0; ox < nw; ++ox) {
        const int sx = xin[(size_t)((flip & 1) ? nw - 1 - ox : ox)];
        unsigned char v = col_v0[(size_t)sx];      // the value at source row 0; transitions above the window map to output row 0 and only toggle it
        int ya = 0;
        seg.clear();
        for (int t = col_start[(size_t)sx]; t < col_start[(size_t)sx + 1]; ++t) {
            const int yb = first[(size_t)trans[(size_t)t]];
            if (flip & 2) seg.push_back(yb - ya);
            else if (!put(v, (unsigned long long)(yb - ya))) { amp::set_error("%s: output capacity %d too small", who, cap); return AMP_ERR_NOMEM; }
            ya = yb;
            v ^= 1;
        }
        if (flip & 2) {
            seg.push_back(nh - ya);
            for (size_t k = seg.size(); k-- > 0; v ^= 1)
                if (!put(v, (unsigned long long)seg[k])) { amp::set_error("%s: output capacity %d too small", who, cap); return AMP_ERR_NOMEM; }
        } else if (!put(v, (unsigned long long)(nh - ya))) { amp::set_error("%s: output capacity %d too small", who, cap); return AMP_ERR_NOMEM; }
    }
    if (mo >= cap) { amp::set_error("%s: output capacity %d too small", who, cap); return AMP_ERR_NOMEM; }
    out[mo++] = (uint32_t)run;
    *m_out = mo;
    return AMP_OK;
}

extern "C" int amp_rle_resize_nearest(const uint32_t* cnts, int m, int h, int w, int nh, int nw, int flip, uint32_t* out, int cap, int* m_out) {
    AMP_REQUIRE(cnts && out && m_out && m > 0 && h > 0 && w > 0 && nh > 0 && nw > 0 && cap > 0, "amp_rle_resize_nearest: bad argument");
    return rle_window_resize("amp_rle_resize_nearest", cnts, m, h, w, 0, 0, h, w, nh, nw, flip ? 1 : 0, out, cap, m_out);
}

extern "C" int amp_rle_crop_resize_nearest(const uint32_t* cnts, int m, int h, int w, int y0, int x0, int ch, int cw, int nh, int nw, int flip,
                                           uint32_t* out, int cap, int* m_out) {
    AMP_REQUIRE(cnts && out && m_out && m > 0 && h > 0 && w > 0 && nh > 0 && nw > 0 && cap > 0 && flip >= 0 && flip <= 3,
                "amp_rle_crop_resize_nearest: bad argument");
    AMP_REQUIRE(y0 >= 0 && x0 >= 0 && ch > 0 && cw > 0 && y0 <= h - ch && x0 <= w - cw,
                "amp_rle_crop_resize_nearest: the window %d x %d at (%d, %d) leaves the %d x %d mask", ch, cw, y0, x0, h, w);
    return rle_window_resize("amp_rle_crop_resize_nearest", cnts, m, h, w, y0, x0, ch, cw, nh, nw, flip, out, cap, m_out);
}

// ---- polygons under a crop ---------------------------------------------------------------------------------------------------------------
// fvcore's CropTransform.apply_polygons intersects every polygon with the crop rectangle (through shapely).  The same REGION from
// Sutherland-Hodgman against the four half-planes, in float64: a non-convex polygon that leaves and re-enters the window comes back as one
// vertex list whose pieces are joined along the window's border (edges walked once in each direction: they enclose nothing, and the
// rasteriser's crossings along them cancel).  An intersection is computed from the edge's start towards its end and held between the two.
extern "C" int amp_polygon_clip_rect(const double* xy, const long long* off, const int* sel, int nsel, double x0, double y0, double x1, double y1,
                                     double* out, long long cap, long long* out_off) {
    AMP_REQUIRE(nsel >= 0 && out_off && (nsel == 0 || (xy && off && sel && out)) && x0 <= x1 && y0 <= y1, "amp_polygon_clip_rect: bad argument");
    std::vector<double> a, b;
    long long o = 0;
    out_off[0] = 0;
    for (int j = 0; j < nsel; ++j) {
        const long long lo = off[sel[j]], hi = off[sel[j] + 1];
        AMP_REQUIRE(lo >= 0 && hi >= lo && (hi - lo) % 2 == 0, "amp_polygon_clip_rect: polygon %d has %lld coordinates", sel[j], hi - lo);
        a.assign(xy + lo, xy + hi);
        for (int plane = 0; plane < 4 && a.size() >= 6; ++plane) {
            const int ax = plane >> 1;                       // 0: a bound on x, 1: a bound on y
            const bool lower = !(plane & 1);
            const double c = ax == 0 ? (lower ? x0 : x1) : (lower ? y0 : y1);
            auto in = [&](const double* p) { return lower ? p[ax] >= c : p[ax] <= c; };
            b.clear();
            const size_t n = a.size() / 2;
            for (size_t i = 0; i < n; ++i) {
                const double* p = &a[2 * ((i + n - 1) % n)];     // the edge that ENDS at vertex i: a polygon inside the window keeps its order
                const double* q = &a[2 * i];
                const bool pi = in(p), qi = in(q);
                if (pi != qi) {
                    const double t = (c - p[ax]) / (q[ax] - p[ax]);
                    double v = p[1 - ax] + t * (q[1 - ax] - p[1 - ax]);
                    v = std::min(std::max(v, std::min(p[1 - ax], q[1 - ax])), std::max(p[1 - ax], q[1 - ax]));
                    double r[2];
                    r[ax] = c; r[1 - ax] = v;
                    b.push_back(r[0]); b.push_back(r[1]);
                }
                if (qi) { b.push_back(q[0]); b.push_back(q[1]); }
            }
            a.swap(b);
        }
        double area2 = 0.0;
        const size_t n = a.size() / 2;
        for (size_t i = 0; i < n; ++i) {
            const size_t k = (i + 1) % n;
            area2 += (a[2 * i] - a[0]) * (a[2 * k + 1] - a[1]) - (a[2 * k] - a[0]) * (a[2 * i + 1] - a[1]);   // relative to vertex 0: exact 0 on a border line
        }
        if (n >= 3 && area2 != 0.0) {
            AMP_REQUIRE(o + (long long)a.size() <= cap, "amp_polygon_clip_rect: more than cap=%lld output coordinates", cap);
            std::copy(a.begin(), a.end(), out + o);
            o += (long long)a.size();
        }
        out_off[j + 1] = o;
    }
    return AMP_OK;
}

// ---- mask_edge_distance (ampis/analyze.py:416-499): argument checks shared with the device path, and the host evaluation ------------------
// For each (ground truth, prediction) pair and its crop [r1:r2, c1:c2]: the squared distance from every false-positive pixel (pred & ~gt) to the
// nearest gt pixel of the crop, and from every false-negative pixel (gt & ~pred) to the nearest pred pixel, queries in row-major order.
// The reference forms a dense [queries x targets x 2] double tensor per pair; here a column pass stores each pixel's distance to the nearest
// target of its own column, and a query walks the columns outward until the column offset alone is no better than what it has: exact
// (integers throughout), memory linear in the crop.
namespace amp {

static int edge_runs_check(const char* which, int p, const uint32_t* c, int m, unsigned long long area) {
    AMP_REQUIRE(m > 0, "amp_mask_edge_distance: pair %d names an empty %s run list", p, which);
    unsigned long long s = 0;
    for (int j = 0; j < m; ++j) s += c[j];
    AMP_REQUIRE(s == area, "amp_mask_edge_distance: the %s runs of pair %d cover %llu pixels, the image has %llu", which, p, s, area);
    return AMP_OK;
}

int edge_distance_check(const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                        const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, const int* box, int n,
                        int h, int w, const uint32_t* fp_d2, unsigned long long fp_cap, const unsigned long long* fp_off, const uint32_t* fn_d2,
                        unsigned long long fn_cap, const unsigned long long* fn_off, std::vector<int>& crop) {
    AMP_REQUIRE(n >= 0 && ng >= 0 && np >= 0 && fp_off && fn_off && (fp_d2 || fp_cap == 0) && (fn_d2 || fn_cap == 0),
                "amp_mask_edge_distance: bad argument");
    AMP_REQUIRE(n == 0 || (gpool && goff && glen && ppool && poff && plen && pair_g && pair_p && box), "amp_mask_edge_distance: null argument");
    AMP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768,
                "amp_mask_edge_distance: image size %d x %d (1 .. 32768 a side: squared distances are 32-bit)", h, w);
    const unsigned long long area = (unsigned long long)h * w;
    std::vector<unsigned char> gok((size_t)ng, 0), pok((size_t)np, 0);          // a run list named by many pairs is summed once
    crop.assign((size_t)n * 4, 0);
    for (int p = 0; p < n; ++p) {
        const int g = pair_g[p], q = pair_p[p];
        AMP_REQUIRE(g >= 0 && g < ng && q >= 0 && q < np, "amp_mask_edge_distance: pair %d = (%d, %d) outside %d x %d masks", p, g, q, ng, np);
        if (!gok[(size_t)g]) { AMP_TRY_STATUS(edge_runs_check("ground-truth", p, gpool + goff[g], glen[g], area)); gok[(size_t)g] = 1; }
        if (!pok[(size_t)q]) { AMP_TRY_STATUS(edge_runs_check("prediction", p, ppool + poff[q], plen[q], area)); pok[(size_t)q] = 1; }
        const int* b = box + 4 * (size_t)p;
        AMP_REQUIRE(b[0] >= 0 && b[2] >= 0 && b[0] <= b[1] && b[2] <= b[3], "amp_mask_edge_distance: box [%d, %d, %d, %d] of pair %d", b[0], b[1], b[2], b[3], p);
        int* c = &crop[4 * (size_t)p];                                            // numpy's slice: an end beyond the image is the image's end
        c[0] = std::min(b[0], h); c[1] = std::min(b[1], h); c[2] = std::min(b[2], w); c[3] = std::min(b[3], w);
    }
    return AMP_OK;
}

// bytes of the crop, row-major, of a column-major run list
static void edge_decode_crop(const uint32_t* c, int m, int h, const int* cr, std::vector<unsigned char>& out) {
    const int H = cr[1] - cr[0], W = cr[3] - cr[2];
    out.assign((size_t)H * W, 0);
    if (H == 0 || W == 0) return;
    const unsigned long long stop = (unsigned long long)cr[3] * h;               // nothing of the crop lies behind its last column
    unsigned long long pos = 0;
    for (int j = 0; j < m && pos < stop; ++j) {
        const unsigned long long s = pos, e = pos + c[j];
        pos = e;
        if (!(j & 1) || e == s) continue;
        const long long first = (long long)(s / (unsigned)h), last = (long long)((e - 1) / (unsigned)h);
        for (long long col = std::max<long long>(first, cr[2]); col <= std::min<long long>(last, cr[3] - 1); ++col) {
            const unsigned long long cb = (unsigned long long)col * h;
            const int ya = std::max((int)(std::max(s, cb) - cb), cr[0]), yb = std::min((int)(std::min(e, cb + h) - cb), cr[1]);
            for (int y = ya; y < yb; ++y) out[(size_t)(y - cr[0]) * W + (size_t)(col - cr[2])] = 1;
        }
    }
}

// squared distance of every pixel of q & ~t to the nearest pixel of t, appended in row-major order
static void edge_nearest(const std::vector<unsigned char>& q, const std::vector<unsigned char>& t, int H, int W, std::vector<int>& colv,
                         std::vector<uint32_t>& out) {
    const int NONE = 1 << 20;
    bool any = false;
    for (size_t i = 0; i < q.size() && !any; ++i) any = q[i] && !t[i];
    if (!any) return;
    colv.assign((size_t)H * W, NONE);                                            // distance to the nearest target of the pixel's own column
    for (int c = 0; c < W; ++c) {
        int d = NONE;
        for (int r = 0; r < H; ++r) { d = t[(size_t)r * W + c] ? 0 : std::min(d + 1, NONE); colv[(size_t)r * W + c] = d; }
        d = NONE;
        for (int r = H - 1; r >= 0; --r) { d = t[(size_t)r * W + c] ? 0 : std::min(d + 1, NONE); int& v = colv[(size_t)r * W + c]; v = std::min(v, d); }
    }
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            if (!q[(size_t)r * W + c] || t[(size_t)r * W + c]) continue;
            uint32_t best = 0xffffffffu;
            const int* row = &colv[(size_t)r * W];
            for (int dc = 0; (uint32_t)dc * (uint32_t)dc < best && (c - dc >= 0 || c + dc < W); ++dc) {
                const uint32_t d2c = (uint32_t)dc * (uint32_t)dc;
                if (c - dc >= 0 && row[c - dc] != NONE) best = std::min(best, (uint32_t)row[c - dc] * (uint32_t)row[c - dc] + d2c);
                if (c + dc < W && row[c + dc] != NONE) best = std::min(best, (uint32_t)row[c + dc] * (uint32_t)row[c + dc] + d2c);
            }
            out.push_back(best);
        }
}

int edge_distance_host(const uint32_t* gpool, const unsigned long long* goff, const int* glen, const uint32_t* ppool, const unsigned long long* poff,
                       const int* plen, const int* pair_g, const int* pair_p, const int* crop, int n, int h, uint32_t* fp_d2,
                       unsigned long long fp_cap, unsigned long long* fp_off, uint32_t* fn_d2, unsigned long long fn_cap, unsigned long long* fn_off) {
    std::vector<uint32_t> fp, fn;                                                // results are handed over whole or not at all
    std::vector<unsigned long long> fpo((size_t)n + 1, 0), fno((size_t)n + 1, 0);
    std::vector<unsigned char> gm, pm;
    std::vector<int> colv;
    for (int p = 0; p < n; ++p) {
        const int* cr = crop + 4 * (size_t)p;
        const int H = cr[1] - cr[0], W = cr[3] - cr[2];
        if (H > 0 && W > 0) {
            edge_decode_crop(gpool + goff[pair_g[p]], glen[pair_g[p]], h, cr, gm);
            edge_decode_crop(ppool + poff[pair_p[p]], plen[pair_p[p]], h, cr, pm);
            edge_nearest(pm, gm, H, W, colv, fp);
            edge_nearest(gm, pm, H, W, colv, fn);
        }
        fpo[(size_t)p + 1] = fp.size();
        fno[(size_t)p + 1] = fn.size();
    }
    if (fp.size() > fp_cap || fn.size() > fn_cap) {
        set_error("amp_mask_edge_distance: %zu false-positive and %zu false-negative pixels, capacities %llu and %llu", fp.size(), fn.size(), fp_cap, fn_cap);
        return AMP_ERR_NOMEM;
    }
    std::copy(fp.begin(), fp.end(), fp_d2);
    std::copy(fn.begin(), fn.end(), fn_d2);
    std::copy(fpo.begin(), fpo.end(), fp_off);
    std::copy(fno.begin(), fno.end(), fn_off);
    return AMP_OK;
}

}  // namespace amp

// ---- region properties (ampis/structures.py:474-514, skimage.measure.regionprops restated): argument checks and tight boxes shared with the
// device path, and the host evaluation.  Per mask 13 exact integers {N, sum r, sum c, sum r^2, sum r c, sum c^2, P1, P2, P3, convex area, 0, 0, 0}:
// the moments in closed form from the runs, the perimeter classes and the hull on a column-major bit plane of the tight box (region_props.h:
// the same word arithmetic as the kernels of region_props.hip).
namespace amp {

int region_props_check(const uint32_t* pool, const unsigned long long* off, const int* len, int n, int h, int w, const long long* bbox,
                       const unsigned long long* vals, std::vector<int>& box) {
    AMP_REQUIRE(n >= 0, "amp_mask_region_props: n = %d", n);
    AMP_REQUIRE(n == 0 || (pool && off && len && bbox && vals), "amp_mask_region_props: null argument");
    AMP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && (unsigned long long)h * w <= (1ull << 30),
                "amp_mask_region_props: image size %d x %d (1 .. 32768 a side, at most 2^30 pixels: the moment sums are 64-bit)", h, w);
    const unsigned long long area = (unsigned long long)h * w;
    box.assign((size_t)n * 4, 0);
    for (int p = 0; p < n; ++p) {
        const uint32_t* c = pool + off[p];
        AMP_REQUIRE(len[p] > 0, "amp_mask_region_props: mask %d has an empty run list", p);
        unsigned long long pos = 0;
        int r0 = h, r1 = -1, c0 = w, c1 = -1;
        for (int j = 0; j < len[p]; ++j) {
            const unsigned long long s = pos, e = pos + c[j];
            pos = e;
            AMP_REQUIRE(e <= area, "amp_mask_region_props: the runs of mask %d cover more than the image's %llu pixels", p, area);
            if (!(j & 1) || e == s) continue;
            const int cf = (int)(s / (unsigned)h), cl = (int)((e - 1) / (unsigned)h);
            c0 = std::min(c0, cf); c1 = std::max(c1, cl);
            if (cf == cl) { r0 = std::min(r0, (int)(s % (unsigned)h)); r1 = std::max(r1, (int)((e - 1) % (unsigned)h)); }
            else { r0 = 0; r1 = h - 1; }                                          // a run that wraps covers the last and the first row
        }
        AMP_REQUIRE(pos == area, "amp_mask_region_props: the runs of mask %d cover %llu pixels, the image has %llu", p, pos, area);
        if (r1 >= 0) { int* b = &box[4 * (size_t)p]; b[0] = r0; b[1] = c0; b[2] = r1 + 1; b[3] = c1 + 1; }
    }
    return AMP_OK;
}

int region_props_host(const uint32_t* pool, const unsigned long long* off, const int* len, const int* box, int n, int h, unsigned long long* vals) {
    std::vector<rp_u64> mask, border;
    std::vector<int> pts;
    for (int p = 0; p < n; ++p) {
        unsigned long long* v = vals + 13 * (size_t)p;
        std::fill(v, v + 13, 0ull);
        const int* b = box + 4 * (size_t)p;
        const int r0 = b[0], c0 = b[1], H = b[2] - b[0], W = b[3] - b[1], pitch = (H + 63) >> 6;
        if (H == 0) continue;
        mask.assign((size_t)W * pitch, 0ull);
        border.assign((size_t)W * pitch, 0ull);
        const uint32_t* c = pool + off[p];
        unsigned long long pos = 0;
        for (int j = 0; j < len[p]; ++j) {
            const unsigned long long s = pos, e = pos + c[j];
            pos = e;
            if (!(j & 1) || e == s) continue;
            rp_run_sums(s, e, (rp_u64)h, v);
            for (unsigned long long col = s / (unsigned)h; col <= (e - 1) / (unsigned)h; ++col) {         // inside the tight box by construction
                const unsigned long long cb = col * (unsigned)h;
                const int ya = (int)(std::max(s, cb) - cb) - r0, yb = (int)(std::min(e, cb + (unsigned)h) - cb) - r0;
                rp_u64* pc = &mask[(size_t)(col - c0) * pitch];
                for (int wv = ya >> 6; wv <= (yb - 1) >> 6; ++wv) {
                    const int lo = std::max(ya - (wv << 6), 0), hi = std::min(yb - (wv << 6), 64);
                    pc[wv] |= (hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
                }
            }
        }
        for (int q = 0; q < W; ++q)
            for (int wv = 0; wv < pitch; ++wv) border[(size_t)q * pitch + wv] = rp_border_at(mask.data(), W, pitch, q, wv);
        for (int q = 0; q < W; ++q)
            for (int wv = 0; wv < pitch; ++wv) {
                if (!border[(size_t)q * pitch + wv]) continue;
                rp_u64 cls[3];
                rp_classify_at(border.data(), W, pitch, q, wv, cls);
                for (int k = 0; k < 3; ++k) v[6 + k] += (unsigned)rp_popc(cls[k]);
            }
        const int np = 2 * W + 1;
        pts.assign((size_t)4 * np, 0);
        int *lo = pts.data(), *hi = lo + np, *sl = hi + np, *su = sl + np;
        for (int i = 0; i < np; ++i) rp_point(i, W, mask.data(), pitch, &lo[i], &hi[i]);
        const int kl = rp_chain(lo, np, +1, sl), ku = rp_chain(hi, np, -1, su);
        long long fill = W;                                                      // sum over the columns of floor(upper / 2) - ceil(lower / 2) + 1
        for (int k = 0; k + 1 < ku; ++k) fill += rp_edge_sum(su[k], hi[su[k]], su[k + 1], hi[su[k + 1]], true);
        for (int k = 0; k + 1 < kl; ++k) fill -= rp_edge_sum(sl[k], lo[sl[k]], sl[k + 1], lo[sl[k + 1]], false);
        v[9] = (unsigned long long)fill;
    }
    return AMP_OK;
}

}  // namespace amp

// ---- all-pairs mask intersection inside groups (ampis/applications/powder.py:80-83, RLE.merge(intersect=True) + RLE.area for every satellite
// against every particle of an image): argument checks that also build the plan (common.h OvPlan), shared with the device path, and the host
// evaluation: the box test, then one walk over both lists of runs for the pairs it leaves.
namespace amp {

static int overlap_plan_pool(const char* which, const uint32_t* pool, const unsigned long long* off, const int* len, const int* first,
                             const int* gh, const int* gw, int ngroups, OvPlan& pl) {
    pl.m.assign((size_t)first[ngroups], OvMask{0, 0, 0, 0, 0, 0, 0});
    for (int g = 0; g < ngroups; ++g) {
        const int h = gh[g];
        const unsigned long long area = (unsigned long long)h * gw[g];
        for (int p = first[g]; p < first[g + 1]; ++p) {
            AMP_REQUIRE(len[p] > 0, "amp_rle_overlap_groups: mask %d of pool %s (group %d) has an empty run list", p, which, g);
            const uint32_t* c = pool + off[p];
            OvMask& e = pl.m[(size_t)p];
            e.ro = (unsigned int)pl.S.size();
            unsigned long long pos = 0, ones = 0;
            int r0 = h, r1 = -1, c0 = gw[g], c1 = -1;
            for (int j = 0; j < len[p]; ++j) {
                const unsigned long long s = pos, t = pos + c[j];
                pos = t;
                AMP_REQUIRE(t <= area, "amp_rle_overlap_groups: the runs of mask %d of pool %s (group %d) cover more than the image's %llu pixels",
                            p, which, g, area);
                if (!(j & 1) || t == s) continue;
                pl.S.push_back((uint32_t)s); pl.E.push_back((uint32_t)t); pl.P.push_back((uint32_t)ones);
                ones += t - s;
                const int cf = (int)(s / (unsigned)h), cl = (int)((t - 1) / (unsigned)h);
                c0 = std::min(c0, cf); c1 = std::max(c1, cl);
                if (cf == cl) { r0 = std::min(r0, (int)(s % (unsigned)h)); r1 = std::max(r1, (int)((t - 1) % (unsigned)h)); }
                else { r0 = 0; r1 = h - 1; }                                      // a run that wraps covers the last and the first row
            }
            AMP_REQUIRE(pos == area, "amp_rle_overlap_groups: the runs of mask %d of pool %s (group %d) cover %llu pixels, the image has %llu",
                        p, which, g, pos, area);
            e.n = (int)(pl.S.size() - e.ro);
            e.area = (unsigned int)ones;
            if (e.n) { e.r0 = r0; e.c0 = c0; e.r1 = r1 + 1; e.c1 = c1 + 1; }
            pl.S.push_back(0xffffffffu); pl.E.push_back(0xffffffffu); pl.P.push_back((uint32_t)ones);
            AMP_REQUIRE(pl.S.size() < (1ull << 31), "amp_rle_overlap_groups: the masks of pool %s have more than 2^31 runs", which);
        }
    }
    return AMP_OK;
}

int overlap_groups_check(const uint32_t* apool, const unsigned long long* aoff, const int* alen, const uint32_t* bpool,
                         const unsigned long long* boff, const int* blen, const int* a_first, const int* b_first, const int* gh, const int* gw,
                         int ngroups, const uint32_t* inter, size_t inter_cap, const unsigned long long* area_a, const unsigned long long* area_b,
                         OvPlan& a, OvPlan& b) {
    AMP_REQUIRE(ngroups >= 0, "amp_rle_overlap_groups: ngroups = %d", ngroups);
    if (ngroups == 0) return AMP_OK;
    AMP_REQUIRE(a_first && b_first && gh && gw, "amp_rle_overlap_groups: null argument");
    AMP_REQUIRE(a_first[0] == 0 && b_first[0] == 0, "amp_rle_overlap_groups: a_first[0] = %d, b_first[0] = %d (group 0 starts at mask 0)",
                a_first[0], b_first[0]);
    unsigned long long total = 0;
    for (int g = 0; g < ngroups; ++g) {
        AMP_REQUIRE(a_first[g + 1] >= a_first[g], "amp_rle_overlap_groups: a_first[%d] = %d is below a_first[%d] = %d", g + 1, a_first[g + 1], g,
                    a_first[g]);
        AMP_REQUIRE(b_first[g + 1] >= b_first[g], "amp_rle_overlap_groups: b_first[%d] = %d is below b_first[%d] = %d", g + 1, b_first[g + 1], g,
                    b_first[g]);
        AMP_REQUIRE(gh[g] >= 1 && gw[g] >= 1 && gh[g] <= 32768 && gw[g] <= 32768 && (unsigned long long)gh[g] * gw[g] <= (1ull << 30),
                    "amp_rle_overlap_groups: image size %d x %d of group %d (1 .. 32768 a side, at most 2^30 pixels)", gh[g], gw[g], g);
        total += (unsigned long long)(a_first[g + 1] - a_first[g]) * (unsigned long long)(b_first[g + 1] - b_first[g]);
    }
    const int na = a_first[ngroups], nb = b_first[ngroups];
    AMP_REQUIRE((na == 0 || (apool && aoff && alen && area_a)) && (nb == 0 || (bpool && boff && blen && area_b)) && (total == 0 || inter),
                "amp_rle_overlap_groups: null argument");
    AMP_REQUIRE(total <= inter_cap, "amp_rle_overlap_groups: inter_cap = %zu, the groups have %llu pairs", inter_cap, total);
    AMP_TRY_STATUS(overlap_plan_pool("A", apool, aoff, alen, a_first, gh, gw, ngroups, a));
    AMP_TRY_STATUS(overlap_plan_pool("B", bpool, boff, blen, b_first, gh, gw, ngroups, b));
    return AMP_OK;
}

int overlap_groups_host(const OvPlan& a, const OvPlan& b, const int* a_first, const int* b_first, int ngroups, uint32_t* inter) {
    size_t out = 0;
    for (int g = 0; g < ngroups; ++g)
        for (int i = a_first[g]; i < a_first[g + 1]; ++i) {
            const OvMask& A = a.m[(size_t)i];
            for (int j = b_first[g]; j < b_first[g + 1]; ++j, ++out) {
                const OvMask& B = b.m[(size_t)j];
                uint32_t sum = 0;
                if (A.n && B.n && A.r0 < B.r1 && B.r0 < A.r1 && A.c0 < B.c1 && B.c0 < A.c1) {
                    const uint32_t *as = &a.S[A.ro], *ae = &a.E[A.ro], *bs = &b.S[B.ro], *be = &b.E[B.ro];
                    for (int p = 0, q = 0; p < A.n && q < B.n;) {
                        const uint32_t lo = std::max(as[p], bs[q]), hi = std::min(ae[p], be[q]);
                        if (hi > lo) sum += hi - lo;
                        if (ae[p] <= be[q]) ++p; else ++q;
                    }
                }
                inter[out] = sum;
            }
        }
    return AMP_OK;
}

}  // namespace amp

// ---- segmentation class map (ampis/analyze.py:589-699, seg_perf_iset): argument checks that also build the plan (common.h OvPlan, entries for
// the masks the pairs name), shared with the device path, and the host evaluation.  TP = OR over the pairs of g & q, FN of g & ~q, FP of
// ~g & q as three column-major bit planes of the image (64 rows a word), painted from the runs of every pair by one walk over both lists; the
// classes of the mode and their run lists then come from the plane words (seg_class_map.h: the same word arithmetic as the kernels of
// seg_class_map.hip).  Memory: three planes of h * w bits and the result, whatever the number of pairs.
namespace amp {

static int seg_plan_mask(const char* which, int pair, int idx, const uint32_t* c, int len, int h, int w, OvPlan& pl, unsigned long long& bounds) {
    AMP_REQUIRE(len > 0, "amp_seg_class_map: pair %d names %s mask %d, which has an empty run list", pair, which, idx);
    const unsigned long long area = (unsigned long long)h * w;
    OvMask& e = pl.m[(size_t)idx];
    e = OvMask{(unsigned int)pl.S.size(), 0, 0, 0, 0, 0, 0};
    unsigned long long pos = 0, ones = 0;
    int r0 = h, r1 = -1, c0 = w, c1 = -1;
    for (int j = 0; j < len; ++j) {
        const unsigned long long s = pos, t = pos + c[j];
        pos = t;
        AMP_REQUIRE(t <= area, "amp_seg_class_map: the runs of %s mask %d (pair %d) cover more than the image's %llu pixels", which, idx, pair, area);
        if (!(j & 1) || t == s) continue;
        pl.S.push_back((uint32_t)s); pl.E.push_back((uint32_t)t); pl.P.push_back((uint32_t)ones);
        ones += t - s;
        const int cf = (int)(s / (unsigned)h), cl = (int)((t - 1) / (unsigned)h);
        c0 = std::min(c0, cf); c1 = std::max(c1, cl);
        if (cf == cl) { r0 = std::min(r0, (int)(s % (unsigned)h)); r1 = std::max(r1, (int)((t - 1) % (unsigned)h)); }
        else { r0 = 0; r1 = h - 1; }                                              // a run that wraps covers the last and the first row
    }
    AMP_REQUIRE(pos == area, "amp_seg_class_map: the runs of %s mask %d (pair %d) cover %llu pixels, the image has %llu", which, idx, pair, pos, area);
    e.n = (int)(pl.S.size() - e.ro);
    e.area = (unsigned int)ones;
    if (e.n) { e.r0 = r0; e.c0 = c0; e.r1 = r1 + 1; e.c1 = c1 + 1; }
    pl.S.push_back(0xffffffffu); pl.E.push_back(0xffffffffu); pl.P.push_back((uint32_t)ones);
    AMP_REQUIRE(pl.S.size() < (1ull << 31), "amp_seg_class_map: the %s masks of the pairs have more than 2^31 runs", which);
    bounds += (unsigned long long)(len - 1);
    return AMP_OK;
}

int seg_class_map_check(const uint32_t* gpool, const unsigned long long* goff, const int* glen, int ng, const uint32_t* ppool,
                        const unsigned long long* poff, const int* plen, int np, const int* pair_g, const int* pair_p, int n, int h, int w,
                        int mode, const uint32_t* counts, unsigned long long counts_cap, const unsigned long long* counts_off,
                        const unsigned long long* pixels, OvPlan& g, OvPlan& p, unsigned long long* need) {
    AMP_REQUIRE(n >= 0 && ng >= 0 && np >= 0, "amp_seg_class_map: n = %d, ng = %d, np = %d", n, ng, np);
    AMP_REQUIRE(mode == 0 || mode == 1, "amp_seg_class_map: mode = %d (0 reduced, 1 all)", mode);
    AMP_REQUIRE(counts && counts_off && pixels, "amp_seg_class_map: null argument");
    AMP_REQUIRE(n == 0 || (gpool && goff && glen && ppool && poff && plen && pair_g && pair_p), "amp_seg_class_map: null argument");
    AMP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768 && (unsigned long long)h * w <= (1ull << 30),
                "amp_seg_class_map: image size %d x %d (1 .. 32768 a side, at most 2^30 pixels)", h, w);
    g.m.assign((size_t)ng, OvMask{0, -1, 0, 0, 0, 0, 0});                         // n = -1: not named by any pair, never read
    p.m.assign((size_t)np, OvMask{0, -1, 0, 0, 0, 0, 0});
    unsigned long long bounds = 0;                                               // every boundary of a class is a boundary of a named run list
    for (int i = 0; i < n; ++i) {
        const int a = pair_g[i], b = pair_p[i];
        AMP_REQUIRE(a >= 0 && a < ng && b >= 0 && b < np, "amp_seg_class_map: pair %d = (%d, %d) outside %d x %d masks", i, a, b, ng, np);
        if (g.m[(size_t)a].n < 0) AMP_TRY_STATUS(seg_plan_mask("ground-truth", i, a, gpool + goff[a], glen[a], h, w, g, bounds));
        if (p.m[(size_t)b].n < 0) AMP_TRY_STATUS(seg_plan_mask("predicted", i, b, ppool + poff[b], plen[b], h, w, p, bounds));
    }
    *need = (unsigned long long)sc_classes(mode) * (bounds + 1);
    if (counts_cap < *need) {
        set_error("amp_seg_class_map: counts_cap = %llu, %llu are needed (classes x (1 + the run boundaries of the masks the pairs name))",
                  counts_cap, *need);
        return AMP_ERR_NOMEM;
    }
    return AMP_OK;
}

// pixels [s, e) of the column-major image into a plane
static void sc_paint(sc_u64* plane, unsigned int s, unsigned int e, int h, int pitch) {
    for (unsigned int col = s / (unsigned)h; col <= (e - 1) / (unsigned)h; ++col) {
        const unsigned int cb = col * (unsigned)h;
        const int ya = (int)(std::max(s, cb) - cb), yb = (int)(std::min(e, cb + (unsigned)h) - cb);
        sc_u64* pc = plane + (size_t)col * pitch;
        for (int wv = ya >> 6; wv <= (yb - 1) >> 6; ++wv) {
            const int lo = std::max(ya - (wv << 6), 0), hi = std::min(yb - (wv << 6), 64);
            pc[wv] |= (hi == 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
        }
    }
}

// every run of A cut by the runs of B: the parts inside B into `in` (or nowhere), the parts outside into `out`
static void sc_split(const OvPlan& pa, const OvMask& A, const OvPlan& pb, const OvMask& B, sc_u64* in, sc_u64* out, int h, int pitch) {
    const uint32_t *as = &pa.S[A.ro], *ae = &pa.E[A.ro], *bs = &pb.S[B.ro], *be = &pb.E[B.ro];
    int k = 0;
    for (int i = 0; i < A.n; ++i) {
        unsigned int pos = as[i];
        const unsigned int e = ae[i];
        while (k < B.n && be[k] <= pos) ++k;
        while (pos < e) {
            if (k < B.n && bs[k] < e) {
                const unsigned int lo = std::max(bs[k], pos), hi = std::min(be[k], e);
                if (lo > pos) sc_paint(out, pos, lo, h, pitch);
                if (in) sc_paint(in, lo, hi, h, pitch);
                pos = hi;
                if (be[k] <= e) ++k;
            } else {
                sc_paint(out, pos, e, h, pitch);
                pos = e;
            }
        }
    }
}

int seg_class_map_host(const OvPlan& g, const OvPlan& p, const int* pair_g, const int* pair_p, int n, int h, int w, int mode, uint32_t* counts,
                       unsigned long long* counts_off, unsigned long long* pixels) {
    const int pitch = (h + 63) >> 6, K = sc_classes(mode);
    const size_t units = (size_t)w * pitch;
    std::vector<sc_u64> planes(3 * units, 0ull);
    sc_u64 *TP = planes.data(), *FN = TP + units, *FP = FN + units;
    for (int i = 0; i < n; ++i) {
        const OvMask& G = g.m[(size_t)pair_g[i]];
        const OvMask& Q = p.m[(size_t)pair_p[i]];
        sc_split(g, G, p, Q, TP, FN, h, pitch);
        sc_split(p, Q, g, G, nullptr, FP, h, pitch);
    }
    std::vector<uint32_t> bnd[7];
    unsigned long long px[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int col = 0; col < w; ++col)
        for (int wv = 0; wv < pitch; ++wv) {
            const size_t u = (size_t)col * pitch + wv;
            const sc_u64 valid = sc_valid(h, wv), tp = TP[u], fn = FN[u], fp = FP[u];
            for (int c = 0; c < 8; ++c) px[c] += (unsigned)sc_popc(sc_code_word(tp, fn, fp, c) & valid);
            const int pb = sc_prev_bit(h, wv);
            const sc_u64 qt = u ? TP[u - 1] >> pb : 0ull, qf = u ? FN[u - 1] >> pb : 0ull, qp = u ? FP[u - 1] >> pb : 0ull;
            const uint32_t base = (uint32_t)col * (uint32_t)h + ((uint32_t)wv << 6);
            for (int k = 0; k < K; ++k) {
                sc_u64 t = sc_transitions(sc_class_word(tp, fn, fp, mode, k) & valid, sc_class_word(qt & 1ull, qf & 1ull, qp & 1ull, mode, k), valid);
                for (; t; t &= t - 1) bnd[k].push_back(base + (uint32_t)sc_ctz(t));
            }
        }
    unsigned long long o = 0;
    const uint32_t area = (uint32_t)((unsigned long long)h * w);
    for (int k = 0; k < K; ++k) {
        counts_off[k] = o;
        uint32_t prev = 0;
        for (uint32_t b : bnd[k]) { counts[o++] = b - prev; prev = b; }
        counts[o++] = area - prev;
    }
    counts_off[K] = o;
    std::copy(px, px + 8, pixels);
    return AMP_OK;
}

}  // namespace amp
