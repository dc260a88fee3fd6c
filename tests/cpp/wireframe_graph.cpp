// wireframe_graph.cpp -- stage 2 of the wireframe, wf_graph of line3dpp_amd/csrc/l3d_wireframe.h, on a case
// file written by tests/test_wireframe_host.py:
//   wireframe_graph <in> <out>
// <in>:  uint32 n, uint32 n_records, double max_distance, double max_extension, n x 6 doubles, n x uint32 line indices,
//        n_records x 32-byte junction records (a, b, sa, sb, gap2) as stage 1 yields them.
// <out>: uint64 sizes of the three arrays, then the junctions, the vertices, the edges and the summary as the C-ABI hands
//        them out; the test compares them with the numpy model byte for byte.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../line3dpp_amd/csrc/l3d_wireframe.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t head[2];
    double thr[2];
    if (std::fread(head, 4, 2, f) != 2 || std::fread(thr, 8, 2, f) != 2) return 4;
    const uint32_t n = head[0], n_rec = head[1];
    std::vector<double> segs(6 * (size_t)n);
    std::vector<uint32_t> line(n);
    std::vector<l3d::WfRecord> rec(n_rec);
    if (std::fread(segs.data(), 48, n, f) != n || std::fread(line.data(), 4, n, f) != n || std::fread(rec.data(), 32, n_rec, f) != n_rec) return 5;
    std::fclose(f);
    for (const l3d::WfRecord& r : rec)
        if (r.a >= n || r.b >= n) return 6;
    l3d::WfGraph g;
    l3d::wf_graph(n, segs.data(), line.data(), thr[0], thr[1], rec.data(), rec.size(), g);
    f = std::fopen(argv[2], "wb");
    if (!f) return 7;
    const uint64_t sizes[3] = {g.junctions.size(), g.vertices.size(), g.edges.size()};
    std::fwrite(sizes, 8, 3, f);
    std::fwrite(g.junctions.data(), sizeof(l3d_wf_junction), g.junctions.size(), f);
    std::fwrite(g.vertices.data(), sizeof(l3d_wf_vertex), g.vertices.size(), f);
    std::fwrite(g.edges.data(), sizeof(l3d_wf_edge), g.edges.size(), f);
    std::fwrite(&g.sum, sizeof(g.sum), 1, f);
    if (std::fclose(f) != 0) return 8;
    std::printf("graph: %zu junctions, %zu vertices, %zu edges\n", g.junctions.size(), g.vertices.size(), g.edges.size());
    return 0;
}
