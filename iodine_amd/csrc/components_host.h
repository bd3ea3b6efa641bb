// Connected components of one segmentation map on the host: the rule of iodine_seg_components (include/iodine_hip.h) in its plainest
// form, behind iodine_seg_components_host.  Plain C++ with no HIP in it, so a test program can compile this file alone.
//
// A raster scan starts a flood fill at every valid pixel that has no component yet: the scan meets a component at its smallest pixel
// first(c), so components are found in the order the rule numbers them.  Every pixel enters the queue once; nothing else loops.
#pragma once
#include <climits>
#include <cstddef>
#include <vector>

// one image; the pointers are the caller's (checked by the entry point), optional outputs may be null
inline void iod_components_host(const unsigned char* seg, int slots, int S, int conn, int min_area, int M, int* labels, int* area_map,
                                int* count, int* per_slot, int* table, unsigned char* clean)
{
    const int P = S * S;
    static const int DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, DY[8] = {0, 0, -1, 1, -1, -1, 1, 1};   // the first four are the 4-neighbours
    std::vector<int> comp(P, -1), queue, first, area;            // comp: index into first / area, in order of first(c)
    queue.reserve(P);
    for (int p = 0; p < P; ++p) {
        if (seg[p] >= slots || comp[p] >= 0) continue;
        const int c = (int)first.size();
        const size_t head0 = queue.size();
        comp[p] = c;
        queue.push_back(p);
        for (size_t head = head0; head < queue.size(); ++head) {
            const int q = queue[head], qx = q % S, qy = q / S;
            for (int n = 0; n < conn; ++n) {
                const int x = qx + DX[n], y = qy + DY[n];
                if (x < 0 || x >= S || y < 0 || y >= S) continue;
                const int r = y * S + x;
                if (seg[r] != seg[p] || comp[r] >= 0) continue;
                comp[r] = c;
                queue.push_back(r);
            }
        }
        first.push_back(p);
        area.push_back((int)(queue.size() - head0));
    }
    const int n_comp = (int)first.size();
    std::vector<int> id(n_comp, -1);
    int kept = 0, small = 0, small_px = 0, invalid = 0;
    if (per_slot) for (int i = 0; i < slots * 4; ++i) per_slot[i] = 0;
    if (table) for (int i = 0; i < M * 8; ++i) table[i] = -1;
    for (int c = 0; c < n_comp; ++c) {
        const int s = seg[first[c]];
        const bool keep = area[c] >= min_area;
        if (keep) id[c] = kept++; else { ++small; small_px += area[c]; }
        if (per_slot) {
            int* ps = per_slot + s * 4;
            ++ps[keep ? 0 : 1];
            if (area[c] > ps[2]) ps[2] = area[c];
            if (!keep) ps[3] += area[c];
        }
        if (table && keep && id[c] < M) {
            int* t = table + id[c] * 8;
            t[0] = s; t[1] = area[c]; t[2] = 0; t[3] = 0; t[4] = INT_MAX; t[5] = INT_MAX; t[6] = -1; t[7] = -1;
        }
    }
    std::vector<int> best(clean ? n_comp : 0, -1);               // small c -> the kept component it takes its slot from
    for (int p = 0; p < P; ++p) {
        const int c = comp[p], x = p % S, y = p / S;
        if (c < 0) {
            ++invalid;
            labels[p] = -1;
            if (area_map) area_map[p] = 0;
            continue;
        }
        labels[p] = id[c];
        if (area_map) area_map[p] = area[c];
        if (table && id[c] >= 0 && id[c] < M) {
            int* t = table + id[c] * 8;
            t[2] += x; t[3] += y;
            if (x < t[4]) t[4] = x;
            if (y < t[5]) t[5] = y;
            if (x > t[6]) t[6] = x;
            if (y > t[7]) t[7] = y;
        }
        if (clean && id[c] < 0)
            for (int n = 0; n < 4; ++n) {
                const int xx = x + DX[n], yy = y + DY[n];
                if (xx < 0 || xx >= S || yy < 0 || yy >= S) continue;
                const int d = comp[yy * S + xx];
                if (d < 0 || id[d] < 0) continue;
                const int b = best[c];
                if (b < 0 || area[d] > area[b] || (area[d] == area[b] && first[d] < first[b])) best[c] = d;
            }
    }
    if (clean)
        for (int p = 0; p < P; ++p) {
            const int c = comp[p];
            clean[p] = (c >= 0 && id[c] < 0 && best[c] >= 0) ? seg[first[best[c]]] : seg[p];
        }
    count[0] = kept; count[1] = small; count[2] = small_px; count[3] = invalid;
}
