// The fused surface as a triangle mesh: marching cubes on the TSDF volume of fusion.hip.  The vertices are endo_fusion_extract's rows --
// every triangle corner of marching cubes lies on a grid edge whose two voxels differ in sign, and the extraction has exactly one row per
// such edge -- so what this file adds is which three rows form each triangle, and a unit normal per row from the tsdf's gradient.  The
// reference has no code for this step; tests/fusion_mesh_restate.py is the numpy float32 statement, matched bit for bit, and the case
// table (fusion_mesh_table.h) is written by tools/gen_fusion_mesh_table.py from the rule stated there.
//
//   cell       the voxels (i..i+1, j..j+1, k..k+1); corner c is voxel (i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)); the case is
//              the sum of (tsdf[c] < 0) << c, surface_edges' own "negative"; a cell takes part when all eight weights are >= min_weight
//   edge       e = 4 a + p: axis a, p = the start corner's bits on the two other axes; its vertex is the row of the start corner's
//              voxel, edge a.  A cell's twelve edges live in the four voxel rows (k, j), (k, j + 1), (k + 1, j), (k + 1, j + 1).
//   count      one block per (k, j): the voxel row's number of rows exactly as fusion_count_kernel counts them, and the cell row's
//              number of triangles; then each scanned by one block (cloud_scan_block), the totals left for the caller's one read
//   vertices   fusion_write_rows with the normals: the rows of endo_fusion_extract, byte for byte
//   faces      one block per cell row, 256 cells per chunk.  A vertex's index is its voxel row's offset plus its rank in that row, so
//              the block recomputes the four rows' edge ballots chunk by chunk (edge_chunk_rank with a running base per row) and
//              leaves each voxel's first index in LDS for its two cells; the voxel just past the chunk ranks as the next chunk's first.
//              No per-voxel index volume goes through HBM: the workspace is 16 bytes per (k, j).  Triangles are ranked inside the
//              chunk by ballots of the three bits of the per-cell counts (0..5) and per-wave sums; cells in i order, a cell's
//              triangles in table order.  The table (4 KiB) is in LDS, read at a lane-varying case.
#include <climits>

#include "fusion_device.h"
#include "fusion_mesh_table.h"

namespace endo {

__constant__ MeshCaseTable d_mesh_cases = kMeshCases;

static_assert(sizeof(kMeshCases.edges) == 16 * kCloudThreads && sizeof(kMeshCases.triangles) == kCloudThreads,
              "a thread copies one case into LDS");

struct MeshParams {
    ExtractParams v;           // offsets: the voxel rows' [nz * ny]; total: the block of totals, [4]: 0, vertices, 0, triangles
    int64_t* tri_offsets;      // [nz * ny], by k * ny + j: the cell rows' (0 triangles where j = ny - 1 or k = nz - 1)
    int32_t* faces;            // [face_capacity][3]
    int64_t face_capacity;
};

// Per voxel row r = y + 2 z of the cell row (k, j), that is row (k + z, j + y), voxel i's bit 2 r: tsdf < 0, and bit 2 r + 1:
// weight >= min_weight; a row outside the grid holds no bits.  With `lo` of voxel i and `hi` of voxel i + 1 the cell's case is
// (lo & 0x55) | ((hi & 0x55) << 1), corner c being x + 2 r, and it takes part when (lo & hi & 0xaa) == 0xaa.
__device__ __forceinline__ int cell_row_signs(const ExtractParams& q, int i, int j, int k) {
    const FusionVolume& g = q.vol;
    int pack = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (j + (r & 1) >= g.ny || k + (r >> 1) >= g.nz) continue;          // (the whole block)
        const int64_t idx = (static_cast<int64_t>(k + (r >> 1)) * g.ny + (j + (r & 1))) * g.nx + i;
        pack |= ((g.tsdf[idx] < 0.0f ? 1 : 0) | (g.weight[idx] >= q.min_weight ? 2 : 0)) << (2 * r);
    }
    return pack;
}

__global__ void __launch_bounds__(kCloudThreads) mesh_count_kernel(const MeshParams q) {
    __shared__ unsigned char s_ntri[kCloudThreads];
    __shared__ int64_t s_tris[kCloudThreads / 64];
    const FusionVolume& g = q.v.vol;
    const int j = blockIdx.x, k = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t row = static_cast<int64_t>(k) * g.ny + j;
    s_ntri[threadIdx.x] = d_mesh_cases.triangles[threadIdx.x];
    __syncthreads();
    // One pass over the row's voxels for both counts.  surface_edges' three tests read the same eight values the cell's case does: the
    // +x neighbour is voxel i + 1 of row 0, the +y and +z neighbours are voxel i of rows 1 and 2, and a neighbour outside the grid
    // holds no bits, so its edge and its cells are absent.  The count is fusion_count_kernel's.
    int cnt = 0;
    int64_t tris = 0;
    for (int i0 = 0; i0 < g.nx; i0 += kCloudThreads) {
        const int i = i0 + threadIdx.x;
        const int lo = i < g.nx ? cell_row_signs(q.v, i, j, k) : 0;
        int hi = __shfl_down(lo, 1, 64);
        if (lane == 63) hi = i + 1 < g.nx ? cell_row_signs(q.v, i + 1, j, k) : 0;          // the next wave's first voxel
        const bool ex = (lo & hi & 2) && ((lo ^ hi) & 1), ey = (lo & (lo >> 2) & 2) && ((lo ^ (lo >> 2)) & 1),
                   ez = (lo & (lo >> 4) & 2) && ((lo ^ (lo >> 4)) & 1);
        cnt += cloud_wave_count(ex) + cloud_wave_count(ey) + cloud_wave_count(ez);
        if ((lo & hi & 0xaa) == 0xaa) tris += s_ntri[(lo & 0x55) | ((hi & 0x55) << 1)];          // (no voxel i + 1: hi = 0)
    }
    cnt = cloud_block_count(cnt);
    if (threadIdx.x == 0) q.v.offsets[row] = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tris += __shfl_down(tris, off, 64);
    if (lane == 0) s_tris[threadIdx.x >> 6] = tris;
    __syncthreads();
    if (threadIdx.x == 0) q.tri_offsets[row] = s_tris[0] + s_tris[1] + s_tris[2] + s_tris[3];
}

__global__ void __launch_bounds__(kScanThreads) mesh_scan_kernel(const MeshParams q) {
    // two blocks, side by side: the voxel rows' counts, the cell rows'
    cloud_scan_block(blockIdx.x == 0 ? q.v.offsets : q.tri_offsets, 1, q.v.vol.ny * q.v.vol.nz, q.v.total + 2 * blockIdx.x);
}

__global__ void __launch_bounds__(kCloudThreads) mesh_vertices_kernel(const ExtractParams q) { fusion_write_rows<true>(q); }

// bits 0..2: surface_edges; bit 3: tsdf < 0; bit 4: weight >= min_weight
__device__ __forceinline__ int voxel_info(const ExtractParams& q, int i, int j, int k) {
    const FusionVolume& g = q.vol;
    const int64_t idx = (static_cast<int64_t>(k) * g.ny + j) * g.nx + i;
    float ta;
    const int edges = surface_edges(q, i, j, k, idx, ta);
    return edges | (ta < 0.0f ? 8 : 0) | (g.weight[idx] >= q.min_weight ? 16 : 0);
}

__global__ void __launch_bounds__(kCloudThreads) mesh_faces_kernel(const MeshParams q) {
    constexpr int kWaves = kCloudThreads / 64;
    __shared__ uint4 s_table[kCloudThreads];                    // a case's sixteen edge ids
    __shared__ unsigned char s_ntri[kCloudThreads];
    __shared__ int s_first[4][kCloudThreads + 1];               // per voxel row of the cell row: the index of a voxel's first row
    __shared__ unsigned char s_info[4][kCloudThreads + 1];      // and its voxel_info; [kCloudThreads]: the voxel just past the chunk
    __shared__ int s_rows[4][kWaves], s_tris[kWaves];           // per-wave sums: rows of each voxel row, triangles
    if (q.v.total[1] > INT_MAX || q.v.total[3] > INT_MAX) return;          // faces are int32 (the whole grid returns)
    const FusionVolume& g = q.v.vol;
    const int j = blockIdx.x, k = blockIdx.y;          // a cell row: j + 1 < ny, k + 1 < nz
    const int64_t cell_row = static_cast<int64_t>(k) * g.ny + j;
    if (q.tri_offsets[cell_row + 1] == q.tri_offsets[cell_row]) return;          // no triangle in this row (row (k, j) + 1 exists: j + 1 < ny)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lower = (1ull << lane) - 1ull;
    s_table[tid] = reinterpret_cast<const uint4*>(d_mesh_cases.edges)[tid];
    s_ntri[tid] = d_mesh_cases.triangles[tid];          // (the chunk's first barrier puts both in front of their readers)
    int64_t base[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) base[r] = q.v.offsets[static_cast<int64_t>(k + (r >> 1)) * g.ny + (j + (r & 1))];
    int64_t tri_at = q.tri_offsets[cell_row];

    for (int i0 = 0; i0 < g.nx - 1; i0 += kCloudThreads) {
        const int i = i0 + tid;
        int rank[4];
        unsigned own = 0;          // the four rows' voxel_info of voxel i, a byte each
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int info = i < g.nx ? voxel_info(q.v, i, j + (r & 1), k + (r >> 1)) : 0;
            const unsigned long long bx = __ballot(info & 1), by = __ballot(info & 2), bz = __ballot(info & 4);
            rank[r] = __popcll(bx & lower) + __popcll(by & lower) + __popcll(bz & lower);
            if (lane == 0) s_rows[r][wave] = __popcll(bx) + __popcll(by) + __popcll(bz);
            s_info[r][tid] = static_cast<unsigned char>(info);
            own |= static_cast<unsigned>(info) << (8 * r);
        }
        if (tid < 4) {
            const int past = i0 + kCloudThreads;
            s_info[tid][kCloudThreads] = past < g.nx ? static_cast<unsigned char>(voxel_info(q.v, past, j + (tid & 1), k + (tid >> 1))) : 0;
        }
        __syncthreads();          // the rows' per-wave sums and every voxel's info in front of their readers

        unsigned next = 0;          // voxel i + 1
        int lo = 0, hi = 0;         // cell_row_signs' packs of voxels i and i + 1
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                if (w < wave) rank[r] += s_rows[r][w];
                total += s_rows[r][w];
            }
            s_first[r][tid] = static_cast<int>(base[r] + rank[r]);
            if (tid == r) s_first[r][kCloudThreads] = static_cast<int>(base[r] + total);          // the next chunk's first
            base[r] += total;
            const unsigned nb = s_info[r][tid + 1];
            next |= nb << (8 * r);
            lo |= static_cast<int>((own >> (8 * r + 3)) & 3u) << (2 * r);
            hi |= static_cast<int>((nb >> 3) & 3u) << (2 * r);
        }
        const int cs = (lo & 0x55) | ((hi & 0x55) << 1);
        const int ntri = (lo & hi & 0xaa) == 0xaa ? s_ntri[cs] : 0;          // (i >= nx - 1: voxel i + 1 has no info, hi = 0)
        const unsigned long long b0 = __ballot(ntri & 1), b1 = __ballot(ntri & 2), b2 = __ballot(ntri & 4);
        int tri_rank = __popcll(b0 & lower) + 2 * __popcll(b1 & lower) + 4 * __popcll(b2 & lower);
        if (lane == 0) s_tris[wave] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
        __syncthreads();          // every voxel's first index and the triangles' per-wave sums in front of their readers; the next
                                  // chunk's s_info and s_rows (written before its first barrier) behind this chunk's readers

        int tri_total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) tri_rank += s_tris[w];
            tri_total += s_tris[w];
        }
        if (ntri) {
            const uint4 entry = s_table[cs];
            const unsigned words[4] = {entry.x, entry.y, entry.z, entry.w};
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const int64_t dst = tri_at + tri_rank + m;
                if (m >= ntri || dst >= q.face_capacity) continue;          // (fewer faces allocated than counted: nothing outside them)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int n = 3 * m + c;
                    const int e = static_cast<int>((words[n >> 2] >> (8 * (n & 3))) & 15u);          // (an edge id of a triangle: 0..11)
                    const int a = e >> 2, p0 = e & 1, p1 = (e >> 1) & 1;
                    const int x = a == 0 ? 0 : p0, y = a == 0 ? p0 : (a == 1 ? 0 : p1), z = a == 2 ? 0 : p1;          // its start corner
                    const int r = y + 2 * z;
                    const unsigned info = ((x ? next : own) >> (8 * r)) & 7u;
                    q.faces[dst * 3 + c] = s_first[r][tid + x] + __popc(info & ((1u << a) - 1u));
                }
            }
        }
        tri_at += tri_total;
    }
    // (s_first and s_tris of the next chunk are written behind its first barrier, which every thread reaches after its faces)
}

static int64_t mesh_row_bytes(int ny, int nz) { return align256(static_cast<int64_t>(ny) * nz * static_cast<int64_t>(sizeof(int64_t))); }

}  // namespace endo

using namespace endo;

extern "C" int endo_fusion_mesh_case(int index, int32_t* edges) {
    if (index < 0 || index > 255) return -1;
    if (edges)
        for (int n = 0; n < 15; ++n) edges[n] = kMeshCases.edges[index][n];
    return kMeshCases.triangles[index];
}

extern "C" int64_t endo_fusion_mesh_workspace_bytes(int nx, int ny, int nz) {
    if (!volume_sizes_ok(nx, ny, nz)) return -1;
    return 2 * mesh_row_bytes(ny, nz);
}

static int mesh_params(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf, const float* weight,
                       const float* color, float min_weight, int64_t* totals, void* workspace, int64_t workspace_bytes, MeshParams& q) {
    const int err = extract_params(origin, voxel_size, nx, ny, nz, tsdf, weight, color, min_weight, totals, workspace, workspace_bytes,
                                   endo_fusion_mesh_workspace_bytes(nx, ny, nz), q.v);
    if (err) return err;
    q.tri_offsets = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + mesh_row_bytes(ny, nz));
    q.faces = nullptr;
    q.face_capacity = 0;
    return 0;
}

extern "C" int endo_fusion_mesh_count(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf,
                                      const float* weight, const float* color, float min_weight, int64_t* totals, void* workspace,
                                      int64_t workspace_bytes, void* stream_) {
    MeshParams q;
    const int err = mesh_params(origin, voxel_size, nx, ny, nz, tsdf, weight, color, min_weight, totals, workspace, workspace_bytes, q);
    if (err) return err;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(nx) * ny * nz * 16.0);
    mesh_count_kernel<<<dim3(ny, nz), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    mesh_scan_kernel<<<2, kScanThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_fusion_mesh_vertices(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf,
                                         const float* weight, const float* color, float min_weight, float* rows, float* normals,
                                         int64_t capacity, int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream_) {
    MeshParams q;
    const int err = mesh_params(origin, voxel_size, nx, ny, nz, tsdf, weight, color, min_weight, totals, workspace, workspace_bytes, q);
    if (err) return err;
    if (capacity < 0 || capacity > INT_MAX || (capacity > 0 && (!rows || !normals))) return ENDO_E_BADARG;
    if (capacity == 0) return 0;
    q.v.rows = rows;
    q.v.normals = normals;
    q.v.capacity = capacity;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(nx) * ny * nz * 8.0 + static_cast<double>(capacity) * 36.0);
    mesh_vertices_kernel<<<dim3(ny, nz), kCloudThreads, 0, stream>>>(q.v);
    ENDO_LAUNCH_CHECK();
    return 0;
}

extern "C" int endo_fusion_mesh_faces(const double* origin, double voxel_size, int nx, int ny, int nz, const float* tsdf,
                                      const float* weight, const float* color, float min_weight, int32_t* faces, int64_t capacity,
                                      int64_t* totals, void* workspace, int64_t workspace_bytes, void* stream_) {
    MeshParams q;
    const int err = mesh_params(origin, voxel_size, nx, ny, nz, tsdf, weight, color, min_weight, totals, workspace, workspace_bytes, q);
    if (err) return err;
    if (capacity < 0 || capacity > INT_MAX || (capacity > 0 && !faces)) return ENDO_E_BADARG;
    if (capacity == 0 || ny < 2 || nz < 2) return 0;          // (no cells: no faces)
    q.faces = faces;
    q.face_capacity = capacity;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ProfScope prof(kProfSmall, stream, 0.0, static_cast<double>(nx) * ny * nz * 8.0 + static_cast<double>(capacity) * 12.0);
    mesh_faces_kernel<<<dim3(ny - 1, nz - 1), kCloudThreads, 0, stream>>>(q);
    ENDO_LAUNCH_CHECK();
    return 0;
}
