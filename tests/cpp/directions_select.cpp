// directions_select.cpp -- stages 0 and 3 of the direction detection, pl_weights of
// line3dpp_amd/csrc/l3d_planes.h and dir_select of l3d_directions.h, on a case file written by
// tests/test_directions_host.py:
//   directions_select <in> <out>
// <in>:  uint32 n, uint32 0, the 64 bytes of l3d_directions_params, n x 6 doubles, n x uint32 line indices and n x 16-byte
//        scores as stage 2 yields them.
// <out>: uint64 sizes of directions, members and seg_directions, then the three arrays and the summary as the C-ABI hands
//        them out, then the n uint64 weights of stage 0; the test compares them with the numpy model byte for byte.
// Exit status 9 where the members recomputed for a tested hypothesis differ from its score.
//   directions_select eigen <in> <out>
// <in>: k x 6 doubles (xx, xy, xz, yy, yz, zz); <out>: k x 3 doubles, dir_largest_eigenvector of each.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../line3dpp_amd/csrc/l3d_directions.h"

static int eigen(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 3;
    std::vector<double> S;
    double row[6];
    while (std::fread(row, 8, 6, f) == 6) S.insert(S.end(), row, row + 6);
    std::fclose(f);
    f = std::fopen(out, "wb");
    if (!f) return 7;
    for (size_t k = 0; k < S.size() / 6; ++k) {
        double v[3];
        l3d::dir_largest_eigenvector(&S[6 * k], v);
        std::fwrite(v, 8, 3, f);
    }
    return std::fclose(f) != 0 ? 8 : 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "eigen") == 0) return eigen(argv[2], argv[3]);
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t head[2];
    l3d_directions_params par;
    if (std::fread(head, 4, 2, f) != 2 || std::fread(&par, sizeof(par), 1, f) != 1) return 4;
    const uint32_t n = head[0];
    std::vector<double> segs(6 * (size_t)n);
    std::vector<uint32_t> line(n);
    std::vector<l3d_dir_score> score(n);
    if (std::fread(segs.data(), 48, n, f) != n || std::fread(line.data(), 4, n, f) != n || std::fread(score.data(), 16, n, f) != n) return 5;
    std::fclose(f);
    l3d::PlWeights w;
    l3d::pl_weights(n, segs.data(), w);
    l3d::DirResult r;
    size_t bad = 0;
    if (l3d::dir_select(n, segs.data(), line.data(), par, w, score.data(), r, &bad)) {
        std::printf("hypothesis %zu: members and score differ\n", bad);
        return 9;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 7;
    const uint64_t sizes[3] = {r.directions.size(), r.members.size(), r.seg_directions.size()};
    std::fwrite(sizes, 8, 3, f);
    auto put = [f](const void* p, size_t size, size_t count) { if (count) std::fwrite(p, size, count, f); };   // (an empty vector's data() may be null)
    put(r.directions.data(), sizeof(l3d_dir_direction), r.directions.size());
    put(r.members.data(), sizeof(l3d_dir_member), r.members.size());
    put(r.seg_directions.data(), 4, r.seg_directions.size());
    put(&r.sum, sizeof(r.sum), 1);
    put(w.q.data(), 8, w.q.size());
    if (std::fclose(f) != 0) return 8;
    std::printf("directions: %zu of %u hypotheses, %zu memberships\n", r.directions.size(), n, r.members.size());
    return 0;
}
