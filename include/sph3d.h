/* sph3d.h — C ABI of libsph3d (hand-written HIP kernels for gfx950 / MI355X).
 *
 * Drop-in boundary for the SPH3D-GCN tf_ops hot path.  Each entry point
 * replaces ONE launcher of the reference (cited per function) and takes
 * exactly what that launcher took — plain ints/floats by value and raw DEVICE
 * pointers — plus a HIP stream.  Differences from the reference launchers, all
 * deliberate:
 *   - every call returns an int status (0 = ok, <0 = SPH3D_E*); the reference
 *     returned void and never checked a launch;
 *   - every call is stream-ordered on `stream` (hipStream_t passed as void*);
 *     nothing synchronises the device (the reference's pool/unpool launchers
 *     called cudaDeviceSynchronize, tf_pool3d_gpu.cu:97,104,111,118);
 *   - outputs do NOT need to be pre-zeroed by the caller: each op fully
 *     defines its outputs (unused neighbour slots = 0, as the reference's
 *     cudaMemset in OpKernel::Compute left them, e.g. tf_nnquery.cpp:100-102);
 *   - all tensors are dense row-major float32 / int32, as in the reference.
 *
 * Notation: B batch, N database/input points, M query/output points,
 * K = nn_sample cap, C in-channels, r depth multiplier, F = n*p*q+1 bins.
 *
 * No torch / TF types appear here.  The Python ops in sph3d_gcn_amd/ bind this
 * file with ctypes; INTEGRATION.md shows the equivalent TF OpKernel binding.
 */
#ifndef SPH3D_H
#define SPH3D_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sph3d_stream_t;   /* hipStream_t */

enum {
    SPH3D_OK = 0,
    SPH3D_EINVAL = -1,      /* bad dimension / attribute (what OP_REQUIRES rejected) */
    SPH3D_EWORKSPACE = -2,  /* workspace too small */
    SPH3D_ELAUNCH = -3,     /* hipGetLastError() != hipSuccess after launch */
    SPH3D_EUNSUPPORTED = -4 /* shape outside what the kernels are built for */
};

/* Library identification. */
/* bumped whenever an exported symbol is removed or changes its signature (2: round 5 removed the sph3d_conv_plan* /
 * sph3d_depthwise_conv3d_lds* entries; additions alone do not bump it) */
#define SPH3D_ABI_VERSION 2
int sph3d_abi_version(void);                 /* == SPH3D_ABI_VERSION of the header the library was built from */
const char* sph3d_last_error(void);          /* thread-local text of the last non-OK status */
const char* sph3d_build_info(void);          /* "gfx950 hipcc <ver> ..." */

/* Test hooks, not modes: the library reads no other environment variable.  Tests set them to reach paths that small inputs
 * do not take.
 *   SPH3D_BWD_HUB_MIN_N=<points>  smallest cloud whose conv gradient takes the hub launches (default 32768; read on every call)
 *   SPH3D_BWD_HUB_T=<edges>       in-edge threshold of a hub source (default 1024, values below 1 count as 1; read on every call)
 *   SPH3D_FPS_FORCE_TIMEOUT=1     the co-operative farthest point sampling pass starts as if timed out, so its repair pass
 *                                 recomputes the samples (any non-zero value; read once per process) */

/* ---- nnquery ------------------------------------------------------------
 * replaces buildSphereNeighborLauncher (tf_ops/nnquery/tf_nnquery_gpu.cu:115-121;
 * kernel cal_nn_binidx :15-65; op BuildSphereNeighbor tf_nnquery.cpp:55-111).
 * database[B,N,3], query[B,M,3] -> nn_index[B,M,K] i32 (ascending database
 * index, first K win, unused = 0), nn_count[B,M] i32 in [1,K],
 * nn_dist[B,M,K] f32 = sqrt(euclidean distance) (sic, :47,:54).
 * Reference semantics reproduced bit-exactly, including the radius-growth
 * chain (:59): query (i,j) is searched with the radius left behind by the
 * previous query of reference-thread (i mod 32, j mod 1024).
 * Growth is bounded: after SPH3D_MAX_GROWTH_PASSES empty passes the query is
 * stored with nn_count = 0 (the reference would spin forever).
 * When no query of a call needs that growth, the radius of a query is a function of its position in the chain alone, and
 * every query is independent (csrc/nngrid.hip): the early positions — radius <= 3 * radius, the queries that would otherwise
 * scan the whole cloud for a handful of hits — are searched over a cell grid, the late ones by an early-stopping scan per
 * query; clouds of at most 1024 points (3 to 32 of them) go through that scan alone, no grid, with a workspace of
 * about a kilobyte.  Whenever some query does need the growth (device-side flag, no host round trip) the chain walk over the cloud
 * (csrc/nnquery.hip) computes the call.  Same rows bit for bit either way.
 * Where the grid lives: the entry points WITH the reference launcher's signature (no workspace argument:
 * sph3d_build_sphere_neighbor[_fixed], sph3d_build_sphere_graph[_ocml]) are conveniences that keep one library-owned
 * device buffer per (device, stream) — hipMalloc on first use, hipFree (a device-wide wait) when it has to grow; a stream
 * that is being captured gets no buffer (no grid: the chain kernel alone).  The `_ws` twins below take the grid's memory
 * from the caller (sph3d_build_sphere_neighbor_workspace bytes, 16-byte aligned): they never allocate, never synchronise and
 * hold no state between calls — what SURVEY 8b asks of every kernel entry; the Python ops of this package call only those.
 * workspace == NULL there: no grid.  sph3d_release_stream_scratch(stream) frees the convenience buffer of `stream` on the
 * current device (call it before destroying the stream), sph3d_release_all_scratch() every buffer of the current device;
 * both return the number of buffers freed. */
#define SPH3D_MAX_GROWTH_PASSES 4096
/* diagnostic: calls so far in this process that went through the cell grid or, on small clouds, through its scan alone */
long long sph3d_nngrid_launches(void);
int sph3d_build_sphere_neighbor(int B, int N, int M, int nn_sample, float radius,
                                const float* database, const float* query,
                                int* nn_index, int* nn_count, float* nn_dist,
                                sph3d_stream_t stream);
/* Same search with a FIXED radius per query — NOT the reference's semantics: every query starts from `radius` (growth by
 * 0.05 only until it has one neighbour; nothing is carried along the reference-thread chain or from cloud to cloud).
 * For clouds much larger than the reference's 8192-point blocks (BASELINE config 5: 65 536 points), where the chain
 * lets the radius reach metres and saturates every row at K. */
int sph3d_build_sphere_neighbor_fixed(int B, int N, int M, int nn_sample, float radius,
                                const float* database, const float* query,
                                int* nn_index, int* nn_count, float* nn_dist,
                                sph3d_stream_t stream);

/* The same two searches with the cell grid's memory from the caller (see above; tf_nnquery.cpp:53-54: the op's Compute
 * allocates every buffer the launcher touches — this is that contract). */
size_t sph3d_build_sphere_neighbor_workspace(int B, int N, int M);
int sph3d_build_sphere_neighbor_ws(int B, int N, int M, int nn_sample, float radius,
                                   const float* database, const float* query,
                                   int* nn_index, int* nn_count, float* nn_dist,
                                   void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_build_sphere_neighbor_fixed_ws(int B, int N, int M, int nn_sample, float radius,
                                   const float* database, const float* query,
                                   int* nn_index, int* nn_count, float* nn_dist,
                                   void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_release_stream_scratch(sph3d_stream_t stream);
int sph3d_release_all_scratch(void);

/* What a range search launches, answered on the host (no device is touched): csrc/nn_plan.hpp states the choice once (nn_plan),
 * every search entry point above and sph3d_build_sphere_graph* below launch what it says, and
 * sph3d_build_sphere_neighbor_workspace reads it.
 *   fixed: 0 the reference's search, 1 the `_fixed` entries;  B, N, M, K (nn_sample), radius as the entry point takes them;
 *   fuse_wanted: 1 for sph3d_build_sphere_graph*;  memory: the front's device memory — SPH3D_NN_MEMORY_CALLER (a `_ws` entry
 *   with a workspace), _LIBRARY (an entry with the reference's signature), _NONE (a `_ws` entry with workspace == NULL; a call
 *   the library finds no buffer for, e.g. under stream capture, is launched as this)
 *   out[SPH3D_NN_PLAN_FIELDS], in this order:
 *     0 front: 0 none, 1 the cell grid (+ the early-stopping scan of the later positions), 2 small clouds: that scan alone.
 *       Counted by sph3d_nngrid_launches() when not 0; fields 1 .. 22 are 0 without a front
 *     1 npos (grid: chain positions it takes; fixed: 1, all queries)   2 nq (queries per cloud in its visiting order)
 *     3 nslices (their slices of 1024)   4 parts (waves of four queries)   5 W (32-bit words of a query's bitmap)
 *     6 build_lds (LDS bytes of nngrid_build_kernel and nngrid_qorder_kernel)   7 search_lds (of nngrid_search_kernel)
 *     8 9 10 workgroups of the build (B), the query order (B nslices), the search (parts of B clouds dealt to the XCDs)
 *     11 j0 (first query of a cloud that nndense_kernel takes: M if none, 0 for small clouds)
 *     12 dparts, 13 dense_lds, 14 dense_grid (nndense_kernel: waves-of-four-queries groups per cloud, LDS bytes, workgroups;
 *     0 when j0 == M)   15 prepare_block (small: threads of nnsmall_prepare_kernel)
 *     16 workspace_bytes, and the byte offsets into it: 17 flag  18 radii and thresholds  19 per-cloud headers  20 cell starts
 *     21 the cloud in cell order  22 the query order (20 .. 22: grid)
 *     23 CPW, 24 MULTI, 25 DEFER: the chain kernel nnquery_sphere_kernel<CPW, MULTI, DEFER, fused> behind the front (CPW 1 with
 *     MULTI)   26 chunkN (points per LDS chunk)   27 groups (workgroups per reference block)   28 chain_grid (workgroups; 0: B or
 *     M is 0, nothing is launched)   29 chain_lds (bytes)   30 grid_done (chain positions the front has finished unless its
 *     flag is up: 0 or 1 << 20)   31 fused (the output passes write bins and segment counts; 0 with fuse_wanted:
 *     sph3d_build_sphere_graph* runs sph3d_spherical_kernel and sph3d_graph_transpose_count behind the search)
 *     32 clear_counts (segments of F counters, B N + 1, that are cleared again in front of the chain kernel when the front's
 *     flag is up; 0: no such launch)
 *   sph3d_build_sphere_neighbor_workspace(B, N, M) is field 16 of (fixed = 1, K = 1, memory = CALLER): at least field 16 for every
 *   K and mode, and equal to it whenever front != 0.
 * -> SPH3D_OK, or SPH3D_EINVAL for a flag outside the above, out == NULL, or arguments the entry point itself rejects (radius,
 *    nn_sample, dimensions, in that order). */
#define SPH3D_NN_MEMORY_NONE 0
#define SPH3D_NN_MEMORY_CALLER 1
#define SPH3D_NN_MEMORY_LIBRARY 2
#define SPH3D_NN_PLAN_FIELDS 33
int sph3d_build_sphere_neighbor_plan(int fixed, int B, int N, int M, int K, float radius, int fuse_wanted, int memory, long long* out);

/* replaces buildCubeNeighborLauncher (tf_nnquery_gpu.cu:123-127; kernel
 * cal_nn_binidx_cube :72-113; op BuildCubeNeighbor tf_nnquery.cpp:116-168).
 * -> nn_index[B,M,K,2] i32 = (database index, cubic bin id), nn_count[B,M]. */
int sph3d_build_cube_neighbor(int B, int N, int M, int grid_size, int nn_sample, float length,
                              const float* database, const float* query,
                              int* nn_index, int* nn_count,
                              sph3d_stream_t stream);

/* Fused graph construction of one level: neighbour search + spherical-kernel bins in ONE kernel, and — when
 * transpose_workspace is given (sph3d_graph_transpose_workspace bytes) — the counting pass of the transposed graph as
 * well (finish it with sph3d_graph_transpose_finish).  Outputs equal, bit for bit, sph3d_build_sphere_neighbor followed by
 * sph3d_spherical_kernel(n, p, q, radius) on the same database / query; shapes whose per-query hit lists do not fit LDS
 * run those kernels one after the other.  filt_index == NULL: no bins (an inter-level graph, n / p / q ignored): the
 * search plus the counting pass for F = 1 (transpose_workspace is then required). */
int sph3d_build_sphere_graph(int B, int N, int M, int nn_sample, float radius, int n, int p, int q,
                             const float* database, const float* query,
                             int* nn_index, int* nn_count, float* nn_dist, int* filt_index,
                             void* transpose_workspace, size_t transpose_workspace_bytes, sph3d_stream_t stream);
/* The same with ROCm's device-library atan2f for the bins (= sph3d_build_sphere_neighbor + sph3d_spherical_kernel_ocml:
 * bit for bit the bins of the reference's own kernel built for this GPU; not reproducible on a CPU). */
int sph3d_build_sphere_graph_ocml(int B, int N, int M, int nn_sample, float radius, int n, int p, int q,
                             const float* database, const float* query,
                             int* nn_index, int* nn_count, float* nn_dist, int* filt_index,
                             void* transpose_workspace, size_t transpose_workspace_bytes, sph3d_stream_t stream);

/* Both of the above with the search's cell grid from the caller (search_workspace: sph3d_build_sphere_neighbor_workspace(B, N, M)
 * bytes, NULL = no grid): no allocation, legal under stream capture.  ocml: 0 = sph3d_build_sphere_graph, 1 = ..._ocml. */
int sph3d_build_sphere_graph_ws(int B, int N, int M, int nn_sample, float radius, int n, int p, int q, int ocml,
                                const float* database, const float* query,
                                int* nn_index, int* nn_count, float* nn_dist, int* filt_index,
                                void* transpose_workspace, size_t transpose_workspace_bytes,
                                void* search_workspace, size_t search_workspace_bytes, sph3d_stream_t stream);

/* ---- buildkernel --------------------------------------------------------
 * replaces sphericalKernelLauncher (tf_ops/buildkernel/tf_buildkernel_gpu.cu:83-89;
 * kernel build_spherical_kernel :20-79; op SphericalKernel tf_buildkernel.cpp:35-99).
 * -> filt_index[B,M,K] i32: 0 = self / unused slot, else
 * 1 + nID + n*pID + n*p*qID.  Requires n>2 even, p>0 even, q>0 (:39-49).
 * atan2f is include/sph3d_atan2f.h (correctly rounded, the same bits on device and in the CPU oracle).
 * sph3d_spherical_kernel_ocml is the same kernel calling ROCm's device-library atan2f: bit-for-bit the bins the
 * reference's own kernel produces when built for this GPU; they differ from the default only for neighbours within an
 * ulp of an angular bin boundary and are not reproducible on a CPU. */
int sph3d_spherical_kernel(int B, int N, int M, int K, int n, int p, int q, float radius,
                           const float* database, const float* query,
                           const int* nn_index, const int* nn_count, const float* nn_dist,
                           int* filt_index,
                           sph3d_stream_t stream);
int sph3d_spherical_kernel_ocml(int B, int N, int M, int K, int n, int p, int q, float radius,
                                const float* database, const float* query,
                                const int* nn_index, const int* nn_count, const float* nn_dist,
                                int* filt_index,
                                sph3d_stream_t stream);

/* ---- convolution --------------------------------------------------------
 * replaces depthwiseConv3dLauncher (tf_ops/convolution/tf_conv3d_gpu.cu:107-113;
 * kernel depthwise_conv3d_forward :7-29; op DepthwiseConv3d tf_conv3d.cpp:47-94).
 * out[b,m,c*r+rho] = (1/cnt) * sum_k in[b,idx_k,c] * filt[bin_k,c,rho].
 * F (= filter.shape[0]) is an extra argument: the filter table is staged in LDS. */
int sph3d_depthwise_conv3d(int B, int N, int M, int F, int C, int r, int K,
                           const int* nn_index, const int* nn_count, const int* bin_index,
                           const float* input, const float* filter, float* output,
                           sph3d_stream_t stream);

/* replaces depthwiseConv3dGradLauncher (tf_conv3d_gpu.cu:115-140; kernels
 * depthwise_input_backward :32-55, depthwise_filter_backward :58-101;
 * op DepthwiseConv3dGrad tf_conv3d.cpp:101-158).
 * grad_input[B,N,C], grad_filter[F,C,r] are fully written.  The wrapper builds the transposed graph
 * (below) in `workspace` (sph3d_depthwise_conv3d_grad_workspace() bytes of device memory) and runs
 * sph3d_depthwise_conv3d_grad_t; callers that keep the transpose across calls use that directly. */
size_t sph3d_depthwise_conv3d_grad_workspace(int B, int N, int M, int F, int C, int r, int K);
int sph3d_depthwise_conv3d_grad(int B, int N, int M, int F, int C, int r, int K,
                                const int* nn_index, const int* nn_count, const int* bin_index,
                                const float* input, const float* filter, const float* grad_output,
                                float* grad_input, float* grad_filter,
                                void* workspace, size_t workspace_bytes,
                                sph3d_stream_t stream);

/* ---- transposed neighbour graph (not in the reference: how its atomic scatters are avoided) ----
 * Every gradient of the path is a scatter over the neighbour graph; libsph3d runs it as a gather over
 * the graph's transpose ("in-edge lists"), built once per graph and reusable by every gradient that
 * uses the same (nn_index, nn_count[, bin_index | weight]).  F = number of filter bins (1 when
 * bin_index is NULL).  In-edges are sorted by (cloud, source point n, bin f):
 *   offsets[B*(N*F+1)]  edges of segment (b,n,f) are entries [offsets[s], offsets[s+1]), s = b*(N*F+1) + n*F + f
 *   ent_key[B*M*K]      m, the graph row (output point) the edge comes from
 *   ent_scale[B*M*K]    1/nn_count[b,m]   (weight[b,m,k] when weight is not NULL)
 * Cloud b's entries fill [offsets[b, 0], offsets[b, N*F]) of its slab [b*M*K, (b+1)*M*K), offsets[b, 0] = b*M*K; the rest of
 * the slab (the slots k >= nn_count of its rows) is not written, nor is active_bins behind its 1 + count words.  A bin id
 * outside [0, F-1] counts for the nearest bin, 0 or F-1, in the offsets and in active_bins.  The order of the entries inside
 * one segment is not defined — except in deterministic mode (sph3d_set_deterministic below), where every build form leaves them
 * in the canonical order of sph3d_graph_canonical_order.  tests/_tgraph_ref.py states all of this in numpy.
 * workspace: sph3d_graph_transpose_workspace() bytes of scratch (segment counters); deterministic mode adds B*M*K words. */
size_t sph3d_graph_transpose_workspace(int B, int N, int M, int K, int F);
int sph3d_graph_transpose(int B, int N, int M, int K, int F,
                          const int* nn_index, const int* nn_count,
                          const int* bin_index /* or NULL */, const float* weight /* or NULL */,
                          int* offsets, int* ent_key, float* ent_scale,
                          int* active_bins /* [F+1] or NULL: count, then the ascending list of the bins that occur */,
                          void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* PACKED entries (round 6): ent_scale == NULL asks sph3d_graph_transpose[_finish[_ordered]] for entry words
 * ent_key[e] = m | nn_count[m] << 24 and no scale array — allowed for un-weighted graphs (weight == NULL) with M <= 2^24 and K <= 255
 * (SPH3D_EINVAL otherwise); every consumer below that takes (ent_key, ent_scale) accepts ent_scale == NULL for such a graph and
 * derives 1 / nn_count[m] from the word (the same correctly rounded division); sph3d_max_pool3d_grad_t masks the row bits itself.
 * Packed entries need nn_count <= K <= 255 in every row: the count takes the word's top eight bits (128..255 set bit 31; the
 * word is formed and decoded in unsigned arithmetic).
 * The two phases of sph3d_graph_transpose on one workspace: segment counts (also produced by sph3d_build_sphere_graph), then
 * scan + fill. */
int sph3d_graph_transpose_count(int B, int N, int M, int K, int F, const int* nn_index, const int* nn_count,
                                const int* bin_index, int want_active, void* workspace, size_t workspace_bytes,
                                sph3d_stream_t stream);
int sph3d_graph_transpose_finish(int B, int N, int M, int K, int F,
                                 const int* nn_index, const int* nn_count, const int* bin_index,
                                 const float* weight, int* offsets, int* ent_key, float* ent_scale, int* active_bins,
                                 void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* The pooling graph of a level = the rows of its intra-level graph at the sampled points (the two tf.gather_nd of
 * models/SPH3D_s3dis.py:68-72) in ONE launch that, with a transpose workspace (sph3d_graph_transpose_workspace(B, N, S, K, 1) bytes;
 * NULL: copy only), also runs the counting phase of the pooling graph's transposed graph (finish it with
 * sph3d_graph_transpose_finish[_ordered]).  pairs[B*S][2] = (cloud, point); out_index [B, S, K], out_count [B, S]. */
int sph3d_gather_rows_count(int B, int N, int S, int K, const int* pairs, const int* nn_index, const int* nn_count,
                            int* out_index, int* out_count, void* transpose_workspace, size_t transpose_workspace_bytes,
                            sph3d_stream_t stream);
/* The same copy with a ROW LINK in place of the counting phase, for sph3d_max_pool3d_grad_rows: no transposed pooling graph is
 * built at all.  first [B, N] (zero-filled by the call) and next [B, S]:
 *   first[b, p] = 0 when no pooled row of cloud b copies intra row p, else (1 + j) for one such row j, with bit 31 set when
 *                 there are more of them (a sampler may return a point more than once);
 *   next[b, j]  = 0, or 1 + the next pooled row that copies the same p.  Every pooled row is reached exactly once.
 * The order of a chain is the order of arrival: SPH3D_EUNSUPPORTED in deterministic mode.  The caller promises
 * pairs[b*S + j][0] == b (a pooled row copies a row of its own cloud; what a sampler's index pairs are); out-of-range pairs are
 * clamped as in sph3d_gather_rows_count.  S < 2^31 - 1. */
int sph3d_gather_rows_link(int B, int N, int S, int K, const int* pairs, const int* nn_index, const int* nn_count,
                           int* out_index, int* out_count, int* first, int* next, sph3d_stream_t stream);
/* sph3d_graph_transpose_finish that also writes sph3d_graph_balanced_order's permutation (order[B*N]; NULL: none) from inside its
 * fill launch: scan (one pass) + fill/order = two launches per graph. */
int sph3d_graph_transpose_finish_ordered(int B, int N, int M, int K, int F,
                                         const int* nn_index, const int* nn_count, const int* bin_index,
                                         const float* weight, int* offsets, int* ent_key, float* ent_scale, int* active_bins,
                                         int* order, void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* A processing order for sph3d_depthwise_conv3d_grad_t (its source_order argument) that balances the in-edges over the
 * gradient kernel's waves: inside windows of 2048 consecutive source points the points are sorted by in-degree (read from
 * `offsets` of the transposed graph with F bins), alternately descending and ascending.  order[B*N], a permutation per
 * cloud; results of the gradient are the same sums in a different order of the filter-gradient partials. */
int sph3d_graph_balanced_order(int B, int N, int F, const int* offsets, int* order, sph3d_stream_t stream);
/* Deterministic mode — process-wide, off by default; sph3d_set_deterministic returns the previous value (0 or 1).  While it is on,
 * every gradient of this library is a pure function of its inputs: the same bits on every run (one device; nothing is claimed
 * for what a collective adds between ranks).
 *   - every build of a transposed graph (sph3d_graph_transpose, _finish[_ordered], the counted workspaces of
 *     sph3d_build_sphere_graph and sph3d_gather_rows_count, the *_grad wrappers that build one internally) ends with the
 *     canonical-order pass below, so the gradient gathers add a segment's terms in one fixed order;
 *   - sph3d_graph_transpose_workspace() (and every workspace size that contains it) is B*M*K words larger: size workspaces
 *     while the mode has the value they will be used with;
 *   - the conv gradient runs no hub launches (float atomics), for any N; SPH3D_BWD_HUB_* are ignored;
 *   - conv gradient shapes with r = 1, odd C and F <= 65 (the generic kernel's while the mode is off) run a fixed-order gather
 *     of their own, and sph3d_depthwise_conv3d_grad_t_workspace() / _grad_workspace() return its slab bytes for them (0 more
 *     than the transposed graph's with the mode off);
 *   - what can only run with float atomics refuses with SPH3D_EUNSUPPORTED: the other conv gradient shapes of the generic kernel
 *     (r outside {1, 2}, F > 65; sph3d_depthwise_conv3d_grad_t, _grad_t_cat, _grad) and sph3d_max_pool3d_grad (use
 *     sph3d_max_pool3d_grad_t).
 * Transposed graphs built while the mode was off keep their arrival order: rebuild them after switching it on. */
int sph3d_set_deterministic(int on);
int sph3d_get_deterministic(void);
/* Canonical order of a transposed graph's entries, in place: inside every segment (cloud, source, bin) ascending by row m, entries
 * of equal m ascending by the factor's bit pattern read as an unsigned 32-bit integer.  Packed entries (ent_scale == NULL) are
 * ordered by word & 0xffffff and the bits of 1 / (word >> 24), so a packed and an un-packed build of one graph list the same
 * (m, factor) sequence.  N, M, K, F as the graph was built with; workspace: sph3d_graph_canonical_order_workspace() bytes. */
size_t sph3d_graph_canonical_order_workspace(int B, int N, int M, int K, int F);
int sph3d_graph_canonical_order(int B, int N, int M, int K, int F, const int* offsets, int* ent_key, float* ent_scale /* NULL: packed */,
                                void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* conv gradients from a prebuilt transposed graph: both gradients in one pass, no float atomics
 * (grad_input gathered in registers; grad_filter accumulated in per-lane registers by persistent workgroups
 * that sweep the clouds of their XCD, one partial table per workgroup written to `workspace` =
 * sph3d_depthwise_conv3d_grad_t_workspace() bytes, then reduced).
 * Non-finite values in grad_output: grad_input is non-finite exactly where the reference's sum has a non-finite term.  grad_filter
 * is non-finite at least there.  With F <= 33, r in {1, 2}, C*r % 4 == 0 and C*r <= 128 the in-edges of a segment (source, bin) are
 * taken in batches of 6 or 8 that run past the segment's end onto in-edges of the same source in other bins, multiplied by a
 * scale of exactly 0: a non-finite grad_output[b, m, j] can then make grad_filter[f, j / r, j % r] NaN (0 * inf, 0 * NaN) in every
 * bin f in which a source named by row m has an in-edge, also where the reference's element is finite.  No other element is
 * affected; the other forms (C*r > 128, two channels per lane, the generic kernel) take exact remainders and deviate nowhere.
 * tests/_conv_ref.py states the op in float64, tests/test_gpu_conv_forms.py holds every launch form to it. */
size_t sph3d_depthwise_conv3d_grad_t_workspace(int B, int N, int F, int C, int r);
int sph3d_depthwise_conv3d_grad_t(int B, int N, int M, int F, int C, int r,
                                  const int* offsets, const int* ent_key, const float* ent_scale,
                                  const int* source_order /* optional [B,N] permutation per cloud: the order in which the sources are swept (NULL = index order) */,
                                  const int* active_bins /* optional, from sph3d_graph_transpose: lets a graph with <= 17 occurring bins run with half the accumulator registers */,
                                  const float* input, const float* filter, const float* grad_output,
                                  float* grad_input, float* grad_filter,
                                  void* workspace, size_t workspace_bytes, sph3d_stream_t stream);

/* ---- fuzzy spherical kernel (not in the reference tree: the interpolated kernel of its authors' follow-up work; fuzzy.hip) ----
 * A neighbour contributes to the (up to) eight bins around it with trilinear weights that sum to 1, so the convolution is a
 * continuous function of the coordinates.  alpha, beta, gamma and the centre rule are those of sph3d_spherical_kernel
 * (tf_buildkernel_gpu.cu:49-68 with include/sph3d_atan2f.h; there is no device-library variant).  Per axis a lower corner and a
 * fraction byte:  azimuth a = alpha - 0.5f, i0 = floorf(a), fa8 = min(255, (int)floorf((a - i0) * 256)), lower sector i0 mod n,
 * upper (i0 + 1) mod n;  elevation j0 = floorf(beta - 0.5f), fb8 likewise, j0 < 0 -> (0, 0), j0 >= p - 1 -> (p - 1, 0), upper
 * min(j0 + 1, p - 1);  the radial axis the same with gamma and q.
 *   filt_index[B,M,K] i32   1 + i0 + n*j0 + n*p*k0 (the hard format applied to the lower corner); 0 for a centre slot and for
 *                           slots k >= nn_count
 *   filt_frac[B,M,K]  i32   fa8 | fb8 << 8 | fg8 << 16; 0 where filt_index is 0
 * Consumers: axis weights (256 - f8, f8); a corner's coefficient is the product of its three axis weights times 2^-24 (exact in
 * fp32, the eight sum to exactly 1); corners that coincide add up; filt_index <= 0 is one term, bin 0 with coefficient 1; bits
 * 24..31 of filt_frac are ignored and every corner bin is clamped to [0, F-1].
 * sph3d_gcn_amd/harness/fuzzy.py states the builder and the convolution in numpy (integers bit for bit, sums in float64). */
int sph3d_fuzzy_spherical_kernel(int B, int N, int M, int K, int n, int p, int q, float radius,
                                 const float* database, const float* query,
                                 const int* nn_index, const int* nn_count, const float* nn_dist,
                                 int* filt_index, int* filt_frac, sph3d_stream_t stream);
/* out[b,m,c*r+rho] = (1/cnt) * sum_{k < min(cnt,K)} in[b,idx_k,c] * sum_t coef_{k,t} * filt[bin_{k,t},c,rho]; rows with cnt = 0
 * give exact 0.  filter[F,C,r] with F = n*p*q + 1 <= 257; any C, r >= 1 (F*r <= 16384), K.  The filter table of a column slice
 * (at most 512 columns and 64 KB) is staged in LDS; wider layers run as several slices. */
int sph3d_fuzzy_depthwise_conv3d(int B, int N, int M, int F, int C, int r, int K, int n, int p, int q,
                                 const int* nn_index, const int* nn_count, const int* filt_index, const int* filt_frac,
                                 const float* input, const float* filter, float* output, sph3d_stream_t stream);
/* Both gradients, fully written, no float atomics:
 *   grad_filter[f,c,rho] = sum over edges and their corners t with bin_t = f of coef_t/cnt_m * in[b,n,c] * grad_output[b,m,c*r+rho]
 *                          — workgroups walk the forward graph by rows and accumulate in LDS tables whose columns each belong to
 *                          one lane; their partial tables (`workspace`, sph3d_fuzzy_depthwise_conv3d_grad_workspace() bytes) are
 *                          added in workgroup order: the same bits on every run, in either mode
 *   grad_input[b,n,c]    = sum over the in-edges of n, sum_rho grad_output[b,m,c*r+rho]/cnt_m * sum_t coef_t * filt[bin_t,c,rho]
 *                          — a gather over (offsets, ent_edge) of sph3d_graph_transpose_finish_edges below, in list order:
 *                          reproducible when the lists were built in deterministic mode. */
size_t sph3d_fuzzy_depthwise_conv3d_grad_workspace(int B, int N, int M, int F, int C, int r, int K);
int sph3d_fuzzy_depthwise_conv3d_grad(int B, int N, int M, int F, int C, int r, int K, int n, int p, int q,
                                      const int* nn_index, const int* nn_count, const int* filt_index, const int* filt_frac,
                                      const int* offsets, const int* ent_edge,
                                      const float* input, const float* filter, const float* grad_output,
                                      float* grad_input, float* grad_filter,
                                      void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* The un-binned transposed graph (F = 1) whose entries name the EDGE, not only its row: ent_edge[B*M*K] holds m*K + k of every
 * in-edge of source (b, n) in [offsets[b*(N+1) + n], offsets[b*(N+1) + n + 1]), so a consumer can read per-slot arrays.  Second
 * phase on a workspace counted by sph3d_graph_transpose_count(..., F = 1, bin_index = NULL, ...) (scan + fill, as
 * sph3d_graph_transpose_finish; workspace: sph3d_graph_transpose_workspace(B, N, M, K, 1) bytes).  The order inside a list is
 * not defined — except in deterministic mode, where it is ascending by edge id. */
int sph3d_graph_transpose_finish_edges(int B, int N, int M, int K, const int* nn_index, const int* nn_count,
                                       int* offsets, int* ent_edge, void* workspace, size_t workspace_bytes,
                                       sph3d_stream_t stream);

/* (transposed graph built with F = 1)  grad_input[B,Nin,C] = sum over in-edges of grad_output[B,Mout,C] * ent_scale: the gradient of
 * avg_pool3d (Nin=N, Mout=M), mean_interpolate and weighted_interpolate (Nin=M coarse, Mout=N fine).
 * Non-finite values: an element with a non-finite term is non-finite, but not always of the reference's kind.  With C <= 128,
 * C % 4 == 0, B * Nin <= 65536 and Mout >= 2 * Nin the in-edges are taken in pairs and an odd last edge is read twice, the
 * second time with scale 0: +-inf in that row gives NaN (0 * inf) where the reference gives +-inf. */
int sph3d_scatter_grad_t(int B, int Nin, int Mout, int C,
                         const int* offsets, const int* ent_key, const float* ent_scale,
                         const float* grad_output, float* grad_input, sph3d_stream_t stream);
/* bytes of workspace the *_grad wrappers below need to build the transposed graph internally
 * (N = number of SOURCE points of the gradient, M = number of graph rows) */
size_t sph3d_scatter_grad_workspace(int B, int N, int M, int K);

/* ---- pooling ------------------------------------------------------------
 * replaces maxPool3dLauncher / maxPool3dGradLauncher / avgPool3dLauncher /
 * avgPool3dGradLauncher (tf_ops/pooling/tf_pool3d_gpu.cu:93-119; kernels :5-90;
 * ops tf_pool3d.cpp:63-234).  max_index[B,M,C] holds the argmax POINT id
 * (first maximum wins, strict >). */
int sph3d_max_pool3d(int B, int N, int M, int C, int K,
                     const int* nn_index, const int* nn_count, const float* input,
                     float* output, int* max_index, sph3d_stream_t stream);
/* (the scatter form: float atomics, SPH3D_EUNSUPPORTED in deterministic mode) */
int sph3d_max_pool3d_grad(int B, int N, int M, int C,
                          const int* max_index, const float* grad_output,
                          float* grad_input, sph3d_stream_t stream);
/* the same gradient as a gather over the TRANSPOSED pooling graph (offsets / ent_key of sph3d_graph_transpose with F = 1 on
 * the pooling graph's nn_index / nn_count): no memset, no float atomics, fixed summation order.  nn_count [B,M]: rows
 * without neighbours carry max_index 0 and their gradient goes to point 0, as in the scatter form. */
int sph3d_max_pool3d_grad_t(int B, int N, int M, int C, const int* offsets, const int* ent_key, const int* nn_count,
                            const int* max_index, const float* grad_output,
                            const float* addend /* optional [B,N,C]: another gradient of the same input, added in (NULL: none) */,
                            float* grad_input, sph3d_stream_t stream);
/* the same gradient for a pooling graph whose M rows are rows of the level's intra graph (sph3d_gather_rows_link), without a
 * transposed pooling graph: offsets / ent_key are the transposed INTRA graph of the N points (F segments per source, packed or
 * plain entries), first / next the pooling graph's row link, nn_count / max_index / grad_output those of the M pooled rows.
 * Same terms per element as sph3d_max_pool3d_grad_t, added in the intra graph's entry order (and a chain's order of arrival).
 * The caller promises that no row of the intra graph lists a point twice (rows of the ball query do not): a pooled row is then
 * met once per source. */
int sph3d_max_pool3d_grad_rows(int B, int N, int M, int C, int F, const int* offsets, const int* ent_key, const int* first,
                               const int* next, const int* nn_count, const int* max_index, const float* grad_output,
                               const float* addend /* optional [B,N,C], as above */, float* grad_input, sph3d_stream_t stream);
/* Non-finite values (C <= 128, C % 4 == 0): neighbours are taken in pairs and the last one of an odd count is read twice, the
 * second time with weight 0, so +-inf in that neighbour's row gives NaN (0 * inf) where the reference gives +-inf.  Only an
 * element that was non-finite anyway is affected. */
int sph3d_avg_pool3d(int B, int N, int M, int C, int K,
                     const int* nn_index, const int* nn_count, const float* input,
                     float* output, sph3d_stream_t stream);
int sph3d_avg_pool3d_grad(int B, int N, int M, int C, int K,
                          const int* nn_index, const int* nn_count, const float* grad_output,
                          float* grad_input,
                          void* workspace /* sph3d_scatter_grad_workspace(B,N,M,K) */, size_t workspace_bytes,
                          sph3d_stream_t stream);

/* ---- unpooling ----------------------------------------------------------
 * replaces meanInterpolateLauncher / meanInterpolateGradLauncher /
 * weightedInterpolateLauncher / weightedInterpolateGradLauncher
 * (tf_ops/unpooling/tf_unpool3d_gpu.cu:87-113; kernels :5-84; ops
 * tf_unpool3d.cpp:64-242).  Here N = fine/output count, M = coarse/input
 * count (the reference's naming): input[B,M,C], nn_index[B,N,K] -> output[B,N,C].
 * Non-finite values, both forward ops (C <= 128, C % 4 == 0): as sph3d_avg_pool3d, +-inf in the last neighbour of an odd count
 * gives NaN where the reference gives +-inf; the element is non-finite either way. */
int sph3d_mean_interpolate(int B, int N, int M, int C, int K,
                           const int* nn_index, const int* nn_count, const float* input,
                           float* output, sph3d_stream_t stream);
int sph3d_mean_interpolate_grad(int B, int N, int M, int C, int K,
                                const int* nn_index, const int* nn_count, const float* grad_output,
                                float* grad_input,
                                void* workspace /* sph3d_scatter_grad_workspace(B,M,N,K) */, size_t workspace_bytes,
                                sph3d_stream_t stream);
int sph3d_weighted_interpolate(int B, int N, int M, int C, int K,
                               const int* nn_index, const int* nn_count,
                               const float* input, const float* weight,
                               float* output, sph3d_stream_t stream);
int sph3d_weighted_interpolate_grad(int B, int N, int M, int C, int K,
                                    const int* nn_index, const int* nn_count,
                                    const float* grad_output, const float* weight,
                                    float* grad_input,
                                    void* workspace /* sph3d_scatter_grad_workspace(B,M,N,K) */, size_t workspace_bytes,
                                    sph3d_stream_t stream);
/* Interpolation of NARROW rows (C <= 16, 16 lanes per row): what the last un-pooling becomes when the layer behind it is a plain
 * product with few outputs (interp(x) W = interp(x W): the logits layer).
 *   output[b,n,:] = base[b,n,:] + sum_k w_k input[b, nn_index[b,n,k], :]     w_k = 1/nn_count[b,n] (weight == NULL) or weight[b,n,k]
 * base [B,N,C] is optional (NULL: zero); a row without neighbours gets its base row unchanged.  The neighbours are summed in the
 * order sph3d_mean_interpolate / sph3d_weighted_interpolate use for C <= 128.  The gradient with respect to `input` gathers over
 * the transposed graph (F = 1), like sph3d_scatter_grad_t: no atomics, fixed order.  Non-finite values in the forward op: as
 * sph3d_avg_pool3d, +-inf in the last neighbour of an odd count (of each 16) gives NaN where the reference gives +-inf. */
int sph3d_interpolate_narrow_supported(int C);
int sph3d_interpolate_narrow(int B, int N, int M, int C, int K,
                             const int* nn_index, const int* nn_count, const float* input,
                             const float* weight, const float* base, float* output, sph3d_stream_t stream);
int sph3d_interpolate_narrow_grad_t(int B, int Nin, int Mout, int C,
                                    const int* offsets, const int* ent_key, const float* ent_scale,
                                    const float* grad_output, float* grad_input, sph3d_stream_t stream);

/* sph3d_pool3d_plan: what an entry of the pooling and un-pooling sections launches for a call (csrc/pool_plan.hpp: pool_plan, which
 * every entry launches from), answered on the host; no device is touched.  Nin: the points gathered FROM (forward) or the gradient's
 * rows; Mout: the rows of the neighbour graph — so for the un-pooling entries Nin = M (coarse) and Mout = N (fine).  K is read by the
 * forward ops, F by _MAX_GRAD_ROWS.  op:
 *   SPH3D_POOL_FWD            sph3d_max_pool3d, _avg_pool3d, _mean_interpolate, _weighted_interpolate (one rule for the three modes)
 *   SPH3D_POOL_SUM_GRAD_T     sph3d_scatter_grad_t and the three *_grad wrappers behind their transpose
 *   SPH3D_POOL_MAX_GRAD       sph3d_max_pool3d_grad (the scatter; its refusal in deterministic mode is the entry's, not the plan's)
 *   SPH3D_POOL_MAX_GRAD_T     sph3d_max_pool3d_grad_t            SPH3D_POOL_MAX_GRAD_ROWS   sph3d_max_pool3d_grad_rows
 *   SPH3D_POOL_NARROW         sph3d_interpolate_narrow           SPH3D_POOL_NARROW_GRAD_T   sph3d_interpolate_narrow_grad_t
 * out[SPH3D_POOL_PLAN_FIELDS], in this order:
 *     0 kernel: SPH3D_POOL_KERNEL_NONE (nothing is launched: B == 0; forward: Mout == 0; _MAX_GRAD: Mout == 0, grad_input is only
 *     cleared), _FWD_HALF gather_fwd_half (C % 4 == 0, C <= 128), _FWD gather_fwd, _BWD_T gather_bwd_t, _BWD_T_SPLIT
 *     gather_bwd_t_split (B Nin <= 65536 and Mout >= 2 Nin), _MAX_BWD maxpool_bwd, _MAX_BWD_T, _MAX_BWD_ROWS, _NARROW_FWD, _NARROW_BWD_T
 *     1 V: channels per lane of the instantiation, 4 (C % 4 == 0) or 1; 0 for maxpool_bwd and the narrow kernels
 *     2 pairs: the two halves of a wave take alternate rows (gather_fwd_half; the split gather at V == 4, C <= 128)
 *     3 passes of a wave over a row's channels, ceil(C / (64 V))   4 ppwg: points per workgroup — 16 from 65536 points (B Mout
 *     forward, B Nin in the max gradients), else 4; gather_bwd_t 16; the split gather 1; narrow 16 rows, 4 sources
 *     5 parts: workgroups' worth of points per cloud, ceil(points / ppwg) (maxpool_bwd: grid.x; narrow: 0)
 *     6 grid.x (the gathers: parts of B clouds dealt to the 8 XCDs; narrow: min(ceil(rows / ppwg), 65536))   7 grid.y (maxpool_bwd: B)
 *     8 block (256)   9 static LDS bytes (the split gather: 4 * 64 V * 4)   10 zero_bytes: bytes of grad_input maxpool_bwd's entry
 *     clears first   11 blocks_wanted = ceil(Mout C / 256), 12 blocks_cap = max(ceil(8192 / B), 1): maxpool_bwd's grid.x is their minimum
 * -> SPH3D_OK, or SPH3D_EINVAL for an op that is none of the above, then the entry's own status and message in the entry's order —
 * bad dimensions, N F >= 2^31 - 1 (_MAX_GRAD_ROWS), B > 65535 (_MAX_GRAD), C > 16 (narrow: SPH3D_EUNSUPPORTED), a grid.x beyond
 * 2^31 - 1 (from B Mout = 2 147 483 641: 2^31 - 7 clouds of one point) — then SPH3D_EINVAL for out == NULL. */
#define SPH3D_POOL_FWD 0
#define SPH3D_POOL_SUM_GRAD_T 1
#define SPH3D_POOL_MAX_GRAD 2
#define SPH3D_POOL_MAX_GRAD_T 3
#define SPH3D_POOL_MAX_GRAD_ROWS 4
#define SPH3D_POOL_NARROW 5
#define SPH3D_POOL_NARROW_GRAD_T 6
#define SPH3D_POOL_KERNEL_NONE 0
#define SPH3D_POOL_KERNEL_FWD_HALF 1
#define SPH3D_POOL_KERNEL_FWD 2
#define SPH3D_POOL_KERNEL_BWD_T 3
#define SPH3D_POOL_KERNEL_BWD_T_SPLIT 4
#define SPH3D_POOL_KERNEL_MAX_BWD 5
#define SPH3D_POOL_KERNEL_MAX_BWD_T 6
#define SPH3D_POOL_KERNEL_MAX_BWD_ROWS 7
#define SPH3D_POOL_KERNEL_NARROW_FWD 8
#define SPH3D_POOL_KERNEL_NARROW_BWD_T 9
#define SPH3D_POOL_PLAN_FIELDS 13
int sph3d_pool3d_plan(int op, int B, int Nin, int Mout, int C, int K, int F, long long* out);

/* ---- sampling -----------------------------------------------------------
 * replaces farthestPointSampleLauncher (tf_ops/sampling/tf_sample_gpu.cu:77-80;
 * kernel farthestpointsampleKernel :7-73; op FarthestPointSample tf_sample.cpp:30-58).
 * inp[b,n,3] -> out[b,m] i32; index 0 first, then argmax of the running
 * minimum squared distance; ties: lower (k mod 1024) wins, then lower k
 * (the reference's thread/tree order, :49,:56-66).  Race-free (the reference
 * has a latent race at :68).  Clouds of 2049 .. 16384 points run a PRUNED form of
 * the same chain (csrc/sample.hip: fps_prune_kernel): spatially sorted blobs of 64
 * points whose distance update is skipped when the new sample provably cannot
 * lower any of their running distances; same samples bit for bit.
 * workspace: sph3d_farthest_point_sample_workspace(b,n,m) bytes (0 when the
 * cloud fits the register-resident kernels, n <= 24576, and for arguments the
 * entry rejects). */
size_t sph3d_farthest_point_sample_workspace(int b, int n, int m);
int sph3d_farthest_point_sample(int b, int n, int m, const float* inp, int* out,
                                void* workspace, size_t workspace_bytes,
                                sph3d_stream_t stream);

/* What sph3d_farthest_point_sample(b, n, m, ...) will launch (csrc/fps_plan.hpp: fps_plan, which the entry launches from and the
 * workspace query sizes from), answered on the host; nothing is launched.  out[SPH3D_FPS_PLAN_FIELDS], in this order:
 *     0 kernel: SPH3D_FPS_NONE (b == 0), _PLAIN fps_reg_kernel<P> (n <= 24576, outside the pruned kernel's range or m == 1),
 *       _PRUNED fps_prune_kernel<P, 16> (2049 <= n <= 16384 and m > 1), _COOP fps_coop_kernel (n > 24576 and b G <= 128, G = ceil(n / 4096)),
 *       _BIG fps_big_kernel alone (n > 24576 otherwise)
 *     1 P (the template's points per thread or lane; 0 for _COOP and _BIG)   2 block (threads per workgroup: 1024, or n rounded up
 *     to 64 below 1024 points)   3 grid (workgroups of the first launch)   4 G (workgroups per cloud: 1 but for _COOP)
 *     5 xcd_local (_COOP: 1 when ceil(b / 8) G <= 16: a cloud's workgroups share an XCD, grid = 8 ceil(b / 8) G and the surplus
 *     workgroups leave; which XCD cloud 0 starts on rotates per launch and is not part of the plan)
 *     6 repair (_COOP: 1, fps_big_kernel is queued behind it and runs only if the co-operative pass raised its error word)
 *     7 big_grid (workgroups of fps_big_kernel, min(b, 64); 0 where it is not launched)
 *     8 workspace_bytes, and the byte offsets into it: 9 the error word   10 the granules [b][2][G] of 8 bytes (_COOP)
 *     11 fps_big_kernel's running distances [big_grid][n] fp32
 * -> SPH3D_OK, or SPH3D_EINVAL with the entry's own message for m <= 0, then n <= 0 or b < 0, then n > 262144, then out == NULL. */
#define SPH3D_FPS_NONE 0
#define SPH3D_FPS_PLAIN 1
#define SPH3D_FPS_PRUNED 2
#define SPH3D_FPS_COOP 3
#define SPH3D_FPS_BIG 4
#define SPH3D_FPS_PLAN_FIELDS 12
int sph3d_farthest_point_sample_plan(int b, int n, int m, long long* out);

/* Keyed inverse-density sampling (csrc/idsample.hip): what inverse_density_sample (tf_ops/sampling/tf_sample.py:27-41, stock TF
 * ops on the global generator in the reference) draws, as a pure function of (nn_dist, nn_count, seed, step, level).
 * nn_dist [B,N,K] fp32, nn_count [B,N] i32 (an intra graph's) -> out [B,S] i32.  Point i of cloud b:
 *   w = (((d[0] + d[1]) + ...) + d[c-1]) / float(c), c = min(nn_count, K): sequential fp32 adds, correctly rounded division, slots
 *       >= c are not used; invalid if c <= 0 or w is not finite or w <= 0;
 *   u = ((hi >> 8) + 1) * 2^-24, hi = high word of feed_draw(feed_cloud_key(seed, step, b), 8 + level, i) (csrc/feed_draws.hpp);
 *   t = sph3d_neglog32(u) / w in fp32 (include/sph3d_log32.h), +inf for an invalid point; key = (bits(t) << 32) | i;
 * out = the low words of the S smallest keys in ascending key order (invalid points last, by index).  harness/idsample.py states
 * this in numpy; the two agree bit for bit.  Clouds of more than sph3d_ids_sample_chunk() points sort in chunks and need
 * sph3d_ids_sample_workspace(B,N) bytes (8-byte aligned; 0 otherwise).  SPH3D_EINVAL: dimensions that are not positive, S > N,
 * level outside 0..7, a null pointer; SPH3D_EUNSUPPORTED: N > 2^20. */
size_t sph3d_ids_sample_workspace(int B, int N);
int sph3d_ids_sample_chunk(void);
int sph3d_ids_sample(int B, int N, int K, int S, const float* nn_dist, const int* nn_count, unsigned long long seed,
                     unsigned long long step, int level, int* out, void* workspace, size_t workspace_bytes,
                     sph3d_stream_t stream);

/* tf.gather_nd with [.., 2] (cloud, point) index pairs, as the model graphs use it on coordinates, neighbour lists and
 * counts of the sampled points (models/SPH3D_s3dis.py:68-72; TensorFlow's stock op in the reference): params is
 * [B, N, row] 4-byte elements, pairs [S, 2] int32, out [S, row].  Out-of-range pairs are clamped. */
int sph3d_gather_nd(int B, int N, long long S, int row, const int* pairs, const void* params, void* out,
                    sph3d_stream_t stream);

/* A permutation of each cloud in which consecutive points are close in space (counting sort by the Morton code of a point's
 * cell in a grid over the cloud's bounding box): order[B,N] int32.  A processing order for gather kernels — it never changes a
 * result, only which rows a workgroup touches together. */
int sph3d_spatial_order(int B, int N, const float* xyz, int* order, sph3d_stream_t stream);

/* ---- pointwise 1x1 feature GEMM (fp32 MFMA) -----------------------------
 * replaces the tf.matmul inside separable_conv3d / pointwise_conv3d /
 * fully_connected (utils/sph3gcn_util.py:146-150, 204-206, 260) -> cuBLAS SGEMM
 * in the reference.  Y[R,Cout] = X[R,Cin] * W[Cin,Cout] (+ bias[Cout]) with an
 * optional fused ELU; exact fp32 (v_mfma_f32_32x32x2_f32).
 * act: 0 = none, 1 = ELU.  bias may be NULL.
 * trans_x / trans_w select the backward products:
 *   dX[R,Cin]  = dY[R,Cout] * W^T      -> sph3d_pointwise_gemm(R, Cout, Cin, dY, W, trans_w=1)
 *   dW[Cin,Cout] = X^T[Cin,R] * dY     -> sph3d_pointwise_gemm_tn(...) */
int sph3d_pointwise_gemm(int R, int Cin, int Cout,
                         const float* X, const float* W, const float* bias, int act,
                         int trans_w, float* Y, sph3d_stream_t stream);
/* How the products (all three, and the statistics variant) run — process-wide, returns the previous mode:
 *   1 (default): bf16 matrix pipe with every fp32 operand cut EXACTLY into three bf16 pieces and the six leading piece products
 *      accumulated in fp32 (csrc/gemm.hip: gemm_split_mfma) — fp32-sized error (<= 2^-23 per product), 2.7x the fp32 MFMA rate;
 *   0: v_mfma_f32_32x32x2_f32, a k-ordered fp32 fmaf chain;  other values: query only.
 * Ragged shapes and misaligned operands take the same kernels with element-wise bounds, in either mode; only the very narrow ones
 * (NN / NT: Cin < 16 or Cout < 32; TN: Cin < 32 or Cout < 32) take the fp32 kernels in mode 1 too. */
int sph3d_pointwise_gemm_mode(int mode);
/* float32 matmul precision of the products on the bf16 matrix pipe — the three levels of torch.set_float32_matmul_precision, as the
 * number of bf16 pieces every fp32 operand is cut into.  Process-wide; 1, 2 or 3 sets the piece count and returns the previous one,
 * any other value only queries.  With rn(x) = fp32 -> bf16 by round-to-nearest-even, widened back to fp32 (on the bit pattern u of a
 * finite x: ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16):
 *   3 (default, "highest"): truncation pieces h, m, l, x = h + m + l exactly, six products — as described at sph3d_pointwise_gemm_mode;
 *   2 ("high")  : h = rn(x), m = rn(x - h) (the subtraction is exact in fp32); per product  m h' + h m' + h h'  is kept.
 *                 Per output element |error| <= c_high * sum_k |x_k| |w_k|,  c_high = 3 * 2^-16 * (1 + 2^-7);
 *   1 ("medium"): h = rn(x); per product  h h'.   |error| <= c_medium * sum_k |x_k| |w_k|,  c_medium = 2^-7 + 2^-16.
 * Piece products are exact in the fp32 accumulator; the accumulation (fp32, small terms first, in the order the launch form already
 * uses) adds its usual share (the tests allow 1e-5 of the same sum).  Non-finite operands never give a finite output; rn rounds the
 * largest finite values to infinity.  A level is a permission: it has effect only where the plan's `pipe` is 1 — products on the fp32
 * pipe (mode 0, and the very narrow ragged shapes above) stay there and are merely more accurate than asked.  It covers
 * sph3d_pointwise_gemm (both trans_w), sph3d_pointwise_gemm_bnstats and sph3d_pointwise_gemm_tn; sph3d_pointwise_gemm_plan,
 * sph3d_pointwise_gemm_mode and every workspace size answer the same at every piece count.  The products inside
 * sph3d_separable_conv3d_fused / _train, sph3d_pointwise_gemm_skinny* and sph3d_pointwise_gemm_cond* keep the default accuracy.
 * Like the mode, this is a process-global read at every launch: do not change it while another thread issues products. */
int sph3d_pointwise_gemm_pieces(int pieces);
/* The launch a product takes, answered on the host (no device is touched): csrc/gemm.hip states the choice once (gemm_plan) and
 * every entry point below launches what it says.
 *   product: SPH3D_GEMM_NN / _NT (sph3d_pointwise_gemm with trans_w = 0 / 1), _NN_STATS (sph3d_pointwise_gemm_bnstats), _TN
 *            (sph3d_pointwise_gemm_tn); R, Cin, Cout as that entry point takes them
 *   aligned: 1 if every operand pointer of the call is 16-byte aligned;  mode: 0 | 1, or -1 for the current process-wide mode;
 *   exchange_ok: 1 if the stream can supply the exchange buffer (0: a stream under capture that has none yet)
 *   out[SPH3D_GEMM_PLAN_FIELDS], in this order:
 *     0 pipe (0 fp32 MFMA, 1 split bf16)   1 bm  2 bn  3 bk (tile extents)   4 guard (element-wise bounds)   5 stats (statistics epilogue)
 *     6 xs (workgroups per tile of the in-kernel exchange, 1: none)   7 nsplit  8 kchunk (the weight gradient's slabs; kchunk: the k
 *     extent of one workgroup, 0: all of k)   9 reduce (1: the slab-sum launch follows)   10 grid (workgroups of the main launch; 0: no
 *     launch, the statistics product outside its shapes)   11 stats_blocks (sph3d_pointwise_gemm_bnstats_blocks; _NN_STATS only)
 * -> SPH3D_OK, or SPH3D_EINVAL for an unknown product, dimensions that are not positive, a flag outside the above or out == NULL. */
#define SPH3D_GEMM_NN 0
#define SPH3D_GEMM_NT 1
#define SPH3D_GEMM_NN_STATS 2
#define SPH3D_GEMM_TN 3
#define SPH3D_GEMM_PLAN_FIELDS 12
int sph3d_pointwise_gemm_plan(int product, int R, int Cin, int Cout, int aligned, int mode, int exchange_ok, int* out);
/* Products whose tile grid is too small to fill the chip run several workgroups per tile that exchange their partial accumulators inside
 * the launch (csrc/gemm.hip); the waiting workgroup's spin is bounded.  -> number of launches that ever gave up waiting
 * (never expected: 0; synchronises with the device; -1 if the counter cannot be read). */
int sph3d_pointwise_gemm_exchange_failures(void);
int sph3d_pointwise_gemm_tn(int R, int Cin, int Cout,
                            const float* X, const float* dY, float* dW,
                            void* workspace, size_t workspace_bytes,
                            sph3d_stream_t stream);
size_t sph3d_pointwise_gemm_tn_workspace(int R, int Cin, int Cout);

/* ---- fused ELU + batch-norm tail of separable_conv3d / pointwise_conv3d --------------------------
 * replaces tf.nn.elu + tf.layers.batch_normalization(momentum=0.99, epsilon=1e-3) applied after the
 * pointwise matmul (utils/sph3gcn_util.py:152-161, 208-220, 328-332; stock TF ops in the reference).
 * y[R,C] is the matmul output; out = (elu(y) - mean) * rstd * gamma + beta with per-channel statistics of
 * elu(y) over the R rows (training) or the running statistics (inference).  `momentum` is the weight of
 * the NEW batch statistics (1 - 0.99).  save_mean / save_rstd [C] feed the backward pass, which needs only
 * y (elu(y) is recomputed).  Requires C % 4 == 0, C <= 1024 and 0 < R <= 2^31 - 1024 = 2147482624 (the
 * statistics pass indexes rows in int and forms R + 1023); all seven sph3d_elu_bn_* entries answer SPH3D_EINVAL
 * to anything else before they read or launch anything, then SPH3D_EWORKSPACE to a missing or short workspace
 * where they take one.  workspace: sph3d_elu_bn_workspace(), defined for every int R. */
size_t sph3d_elu_bn_workspace(int R, int C);
int sph3d_elu_bn_forward(int R, int C, const float* y, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps, int training,
                         float* out, float* save_mean, float* save_rstd,
                         void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_elu_bn_backward(int R, int C, const float* y, const float* dout, const float* gamma,
                          const float* save_mean, const float* save_rstd, int training,
                          float* dy, float* dgamma, float* dbeta,
                          void* workspace, size_t workspace_bytes, sph3d_stream_t stream);

/* ---- fused forward of a layer tail: GEMM whose epilogue emits the batch-norm statistics' partial sums ---------------
 * (utils/sph3gcn_util.py:146-161: tf.matmul -> ELU -> tf.layers.batch_normalization; SURVEY 8f.3, first half.)
 * sph3d_pointwise_gemm_bnstats writes Y = X W (+ bias; raw, the backward pass needs it) and partial[nblk][2][Cout] = per row block
 * sum elu(y), sum elu(y)^2; nblk = sph3d_pointwise_gemm_bnstats_blocks(R, Cin, Cout), 0 when the shape does not qualify
 * (whole 128/64-row tiles, Cout a multiple of 64 — of 128 above 64 —, Cin a multiple of 16; 16-byte aligned operands):
 * then run sph3d_pointwise_gemm and sph3d_elu_bn_forward.  sph3d_elu_bn_forward_partials is sph3d_elu_bn_forward
 * (training mode) without its statistics pass over Y. */
int sph3d_pointwise_gemm_bnstats_blocks(int R, int Cin, int Cout);
int sph3d_pointwise_gemm_bnstats(int R, int Cin, int Cout, const float* X, const float* W, const float* bias /* [Cout] or NULL */,
                                 float* Y, float* partial, sph3d_stream_t stream);
int sph3d_elu_bn_forward_partials(int R, int C, int nblk, const float* partial, const float* y, const float* gamma,
                                  const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                  float* out, float* save_mean, float* save_rstd, sph3d_stream_t stream);

/* ---- the same tail with training-mode statistics over the rows of SEVERAL ranks ---------------------------
 * sph3d_elu_bn_forward / _backward cut at the statistics: `*_sums` leaves this rank's per-channel sums on the device as doubles,
 * the caller adds the other ranks' buffers on top (one all-reduce, ordered on `stream`), `*_apply` forms the statistics from the
 * summed buffer and runs the apply pass.  Nothing returns to the host, nothing is allocated, no entry point synchronises; with the
 * buffer left as `*_sums` wrote it the pair computes sph3d_elu_bn_forward / _backward (training) bit for bit.  Same shapes
 * (C % 4 == 0, C <= 1024, 0 < R <= 2^31 - 1024: every rank needs at least one row); workspace: sph3d_elu_bn_workspace(R, C) of the rank's own R. */
/* sums [2C + 1] (double) = sum elu(y), sum elu(y)^2 per channel, then the row count R.  partial == NULL: the statistics pass over y
 * runs here (needs the workspace; nblk is ignored); else partial[nblk][2][C] as sph3d_elu_bn_forward_partials takes it (y and the
 * workspace are not read). */
int sph3d_elu_bn_forward_sums(int R, int C, int nblk, const float* partial, const float* y, double* sums,
                              void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* sums: the summed [2C + 1] buffer.  mean = S / Rg, var = max(Q / Rg - mean^2, 0) (double); writes save_mean / save_rstd, updates
 * the running statistics with the biased variance (NULL: not kept), writes the global row count Rg to count [1] (double, read by
 * sph3d_elu_bn_backward_apply on the device), then out = (elu(y) - mean) * rstd * gamma + beta over this rank's R rows. */
int sph3d_elu_bn_forward_apply(int R, int C, const double* sums, const float* y, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float momentum, float eps,
                               float* out, float* save_mean, float* save_rstd, double* count, sph3d_stream_t stream);
/* dgamma / dbeta [C]: this rank's sums in fp32 — they stay local, the gradient all-reduce adds the ranks' like any parameter
 * gradient.  sums [2C] (double) = sum dout, sum dout * zhat per channel. */
int sph3d_elu_bn_backward_sums(int R, int C, const float* y, const float* dout, const float* save_mean, const float* save_rstd,
                               float* dgamma, float* dbeta, double* sums,
                               void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
/* sums: the summed [2C] buffer; count: what sph3d_elu_bn_forward_apply wrote.  dy over this rank's R rows with the two mean terms
 * S / Rg, Q / Rg. */
int sph3d_elu_bn_backward_apply(int R, int C, const double* sums, const double* count, const float* y, const float* dout,
                                const float* gamma, const float* save_mean, const float* save_rstd, float* dy,
                                void* workspace, size_t workspace_bytes, sph3d_stream_t stream);

/* ---- fused separable convolution for inference ---------------------------------------------------------
 * The whole layer of utils/sph3gcn_util.py:134-161 with is_training=False in one kernel: DepthwiseConv3d
 * (tf_conv3d.cpp:34-107 / tf_conv3d_gpu.cu:7-29) -> matmul with pointwise_weights[C*r][Cout] -> + bias[Cout] (NULL: none)
 * -> act (0 none | 1 ELU) -> y*scale[Cout] + shift[Cout] (NULL: identity; batch norm with the moving statistics is
 * scale = gamma / sqrt(moving_var + eps), shift = beta - moving_mean*scale).  output [B, M, Cout]; the [B, M, C*r] depthwise
 * tensor is never written.  Shapes: r in {1, 2}; C a multiple of 4, at most 128 or a multiple of 128 up to 4096; Cout a multiple of
 * 16 up to 512; F <= 254 and few enough bins that the filter table (a 128-channel slice of it) and one 16-point tile fit the CU's
 * 160 KB of LDS (F <= 142 beside 256 depthwise channels); N <= 2^24 and N*C*4 < 2^32.  Three kernels share them: where C <= 128,
 * C*r <= 256 and Cout is a power of two up to 256 the barrier-free ring kernel of the training entry below, else for Cout <= 128
 * the small kernel (pointwise weights resident in registers), else the general one (weights streamed per 128-channel slice).
 * sph3d_separable_conv3d_fused_supported() -> 1 | 0, and the call returns SPH3D_EUNSUPPORTED outside them (run
 * sph3d_depthwise_conv3d_forward + sph3d_pointwise_gemm then). */
int sph3d_separable_conv3d_fused_supported(int N, int F, int C, int r, int K, int Cout);
int sph3d_separable_conv3d_fused(int B, int N, int M, int F, int C, int r, int K, int Cout, int act,
                                 const int* nn_index, const int* nn_count, const int* bin_index, const float* input,
                                 const float* depthwise_filter, const float* pointwise_weights, const float* bias,
                                 const float* scale, const float* shift, float* output, sph3d_stream_t stream);

/* ---- fused separable convolution for TRAINING ("BN stats as a side reduction") ----------------------------------
 * The layer of utils/sph3gcn_util.py:134-161 with is_training=True up to the batch-norm statistics, in one barrier-free kernel
 * (csrc/sepring.hip): DepthwiseConv3d (tf_conv3d.cpp:34-107 / tf_conv3d_gpu.cu:7-29) -> matmul with
 * pointwise_weights[C*r][Cout] (+ bias[Cout], NULL: none).  Writes
 *   depthwise_output [B, M, C*r]   the depthwise tensor (operand of the weight gradient; not re-read by the forward pass),
 *   y                [B, M, Cout]  the raw product (what sph3d_elu_bn_backward needs),
 *   partial          [nblk][2][Cout]  per (workgroup, wave group) sum elu(y), sum elu(y)^2 over its rows — the layout
 *                    sph3d_elu_bn_forward_partials consumes; nblk = sph3d_separable_conv3d_train_blocks(Cout).
 * Shapes: r in {1, 2}, C % 4 == 0, C <= 128, C*r <= 256, Cout in {16, 32, 64, 128, 256}, F <= 254
 * (sph3d_separable_conv3d_train_supported() -> 1 | 0; SPH3D_EUNSUPPORTED otherwise: run sph3d_depthwise_conv3d +
 * sph3d_pointwise_gemm_bnstats).  The same kernel without the two extra outputs serves sph3d_separable_conv3d_fused on
 * these shapes.  sph3d_separable_conv3d_ring_failures(): 1 if a launch ever gave up waiting (never expected; synchronises). */
/* The launch either entry point takes, answered on the host (no device is touched): csrc/sepconv.hpp states the choice once
 * (sep_plan) and both entry points launch what it says.  train: 1 sph3d_separable_conv3d_train, 0 sph3d_separable_conv3d_fused;
 * the dimensions as that entry point takes them.
 *   out[SPH3D_SEP_PLAN_FIELDS], in this order:
 *     0 kernel (0 the shape is unsupported: every field is 0; 1 ring, 2 small, 3 general)   1 R (depth multiplier)   2 LPE (lanes per
 *     edge of the gather: 16 for C <= 64, else 32)   3 KT (ring, small: k groups of 16 the kernel is instantiated for; general: 0)
 *     4 RBK (general: 16-point row blocks per tile; else 0)   5 RBK by the point count alone, before many bins lower it (general; else 0)
 *     6 NB (ring: slots)   7 G (ring: wave groups)   8 dynamic LDS bytes   9 grid (workgroups; 0: nothing is launched — inference with
 *     B == 0 or M == 0; training still launches)   10 stats_blocks (training: sph3d_separable_conv3d_train_blocks; else 0)
 * -> SPH3D_OK, or SPH3D_EINVAL for out == NULL, train outside {0, 1}, negative B or M, or N, F, C, K, Cout that are not positive. */
#define SPH3D_SEP_PLAN_FIELDS 11
int sph3d_separable_conv3d_plan(int train, int B, int N, int M, int F, int C, int r, int K, int Cout, int* out);
int sph3d_separable_conv3d_train_supported(int N, int F, int C, int r, int K, int Cout);
int sph3d_separable_conv3d_train_blocks(int Cout);
int sph3d_separable_conv3d_train(int B, int N, int M, int F, int C, int r, int K, int Cout,
                                 const int* nn_index, const int* nn_count, const int* bin_index, const float* input,
                                 const float* depthwise_filter, const float* pointwise_weights, const float* bias,
                                 float* depthwise_output, float* y, float* partial, sph3d_stream_t stream);
int sph3d_separable_conv3d_ring_failures(void);

/* ---- the 1x1 layer with few outputs over two operand halves (the logits layer) ------------------------------------------------
 * tf.concat((unpooled, skip), axis=2) followed by pointwise_conv3d to num_cls outputs (models/SPH3D_s3dis.py:104-108,
 * utils/sph3gcn_util.py:166-222) without materialising the concatenation:
 *   sph3d_pointwise_gemm_skinny     Y[R,N] = A1[R,K1] W[0:K1] + A2[R,K2] W[K1:K1+K2] (+ bias[N] or NULL); A2 = NULL with K2 = 0: one operand
 *   sph3d_pointwise_gemm_skinny_tn  dW[K1+K2,N] = [A1 | A2]^T dY   (workspace: ..._tn_workspace bytes; fixed summation order)
 * N <= 16, K1 and K2 multiples of 16, K1 + K2 <= 256 in at most four started groups of 64 channels (ceil(K1/64) + ceil(K2/64) <= 4),
 * 16-byte aligned operands (..._supported() -> 1 | 0; SPH3D_EUNSUPPORTED
 * otherwise: concatenate and call sph3d_pointwise_gemm / _tn).  The input gradients are sph3d_pointwise_gemm(trans_w = 1) with
 * the matching rows of W, once per operand half. */
int sph3d_pointwise_gemm_skinny_supported(int R, int K1, int K2, int N);
int sph3d_pointwise_gemm_skinny(int R, int K1, int K2, int N, const float* A1, const float* A2, const float* W, const float* bias,
                                float* Y, sph3d_stream_t stream);
size_t sph3d_pointwise_gemm_skinny_tn_workspace(int R, int K1, int K2, int N);
int sph3d_pointwise_gemm_skinny_tn(int R, int K1, int K2, int N, const float* A1, const float* A2, const float* dY, float* dW,
                                   void* workspace, size_t workspace_bytes, sph3d_stream_t stream);

/* ---- the category-conditioned logits layer of the one-hot ShapeNet model ------------------------------------------------------
 * models/SPH3D_shapenet_onehot.py:105-119: tf.concat((mlp2 output, mlp1 features), axis=2), tf.concat with a [B, P, T] tile of
 * tf.one_hot(cls_label), then pointwise_conv3d to num_cls outputs — without the tile or either concatenation.  The one-hot block
 * times its T rows of W is one row of W per cloud:
 *   sph3d_pointwise_gemm_cond       Y[b*P + p, :] = A1[b*P + p, :] W[0:K1] + A2[b*P + p, :] W[K1:K1+K2] + W[K1+K2+cat[b], :] (+ bias)
 *                                   A1 [B*P, K1], A2 [B*P, K2] (NULL with K2 = 0), W [K1+K2+T, N], bias [N] or NULL, cat [B] int32;
 *                                   a category outside [0, T) selects no row (tf.one_hot gives zeros there)
 *   sph3d_pointwise_gemm_cond_grad  dT[c, :] = sum over the clouds b with cat[b] == c and over p of dY[b*P + p, :]  ([T, N]: the
 *                                   gradient of W[K1+K2:]; rows of categories no cloud has are exactly 0, categories outside
 *                                   [0, T) are skipped) and, unless dbias == NULL, dbias[N] = the sum over all rows.  Two
 *                                   launches in a fixed summation order, no floating-point atomics
 *                                   (workspace: ..._cond_grad_workspace bytes).
 * Shapes: K1 >= 16 and K2 >= 0 multiples of 16, K1 + K2 <= 128, N <= 64, T <= 4096, B*P + 15 fits an int (the gradient: B <= 65535),
 * 16-byte aligned operands; ..._cond_supported() -> 1 | 0.  Dimensions that are not positive, B*P past an int, a NULL operand or
 * a workspace that is too small give SPH3D_EINVAL, any other shape outside the above SPH3D_EUNSUPPORTED (concatenate and call
 * sph3d_pointwise_gemm then); both before any launch.  The other gradients are existing entries: dA1 / dA2 =
 * sph3d_pointwise_gemm(trans_w = 1) with the matching rows of W, dW[0:K1] and dW[K1:K1+K2] = sph3d_pointwise_gemm_tn per half. */
int sph3d_pointwise_gemm_cond_supported(int B, int P, int K1, int K2, int N, int T);
int sph3d_pointwise_gemm_cond(int B, int P, int K1, int K2, int N, int T, const float* A1, const float* A2, const float* W,
                              const float* bias, const int* cat, float* Y, sph3d_stream_t stream);
size_t sph3d_pointwise_gemm_cond_grad_workspace(int B, int P, int N, int T);
int sph3d_pointwise_gemm_cond_grad(int B, int P, int N, int T, const float* dY, const int* cat, float* dT, float* dbias,
                                   void* workspace, size_t workspace_bytes, sph3d_stream_t stream);

/* ---- the depthwise convolution over a channel concatenation that is never materialised --------------------------------------
 * DepthwiseConv3d / DepthwiseConv3dGrad (tf_conv3d.cpp:34-107, :109-205) applied to tf.concat((input_a, input_b), axis=2)
 * (models/SPH3D_s3dis.py:100-104: a decoder level's un-pooled features and the encoder's skip features): input_a [B,N,Ca],
 * input_b [B,N,Cb], filter [F, Ca+Cb, r], output [B,M,(Ca+Cb)*r]; the gradient writes grad_a [B,N,Ca] and grad_b [B,N,Cb]
 * (workspace: sph3d_depthwise_conv3d_grad_t_workspace(B, N, F, Ca+Cb, r)).  The kernels' channel slices are 256 outputs wide and
 * must lie inside one input: Ca*r a multiple of 256, Ca+Cb > 128, (Ca+Cb) % 4 == 0, r in {1,2}, F <= 33
 * (..._cat_supported() -> 1 | 0; SPH3D_EUNSUPPORTED otherwise: concatenate and call the plain entries). */
int sph3d_depthwise_conv3d_cat_supported(int F, int Ca, int Cb, int r);
int sph3d_depthwise_conv3d_cat(int B, int N, int M, int F, int Ca, int Cb, int r, int K, const int* nn_index, const int* nn_count,
                               const int* bin_index, const float* input_a, const float* input_b, const float* filter, float* output,
                               sph3d_stream_t stream);
int sph3d_depthwise_conv3d_grad_t_cat(int B, int N, int M, int F, int Ca, int Cb, int r, const int* offsets, const int* ent_key,
                                      const float* ent_scale, const int* source_order, const int* active_bins, const float* input_a,
                                      const float* input_b, const float* filter, const float* grad_output, float* grad_a,
                                      float* grad_b, float* grad_filter, void* workspace, size_t workspace_bytes,
                                      sph3d_stream_t stream);
/* The launch a depthwise convolution or its gradient takes, answered on the host (no device is touched): csrc/conv_plan.hpp states
 * the choice once (conv_plan) and every entry point above launches what it says; the two workspace queries and
 * sph3d_depthwise_conv3d_cat_supported read it.
 *   op: SPH3D_CONV_FWD (sph3d_depthwise_conv3d), _FWD_CAT (sph3d_depthwise_conv3d_cat), _GRAD_T (sph3d_depthwise_conv3d_grad_t, and
 *       through it sph3d_depthwise_conv3d_grad), _GRAD_T_CAT (sph3d_depthwise_conv3d_grad_t_cat)
 *   B, N, M, F, r as that entry point takes them; Ca, Cb: the channels (one input: C and 0); K: the forward ops' (the gradients
 *   have none: ignored);  deterministic: 0 | 1, or -1 for the current mode;  active_given: 1 if the gradient's active_bins is
 *   not NULL (forward: ignored).  The hub hooks SPH3D_BWD_HUB_MIN_N / SPH3D_BWD_HUB_T are read as a call reads them.
 *   out[SPH3D_CONV_PLAN_FIELDS], in this order:
 *     0 kernel: 0 none — nothing is launched (forward: B == 0 or M == 0; gradient: B == 0, grad_filter is zero-filled) and every
 *       field but 21 is 0;  1 dwconv_fwd_multi  2 dwconv_fwd_row  3 dwconv_fwd_generic  4 dwconv_bwd_t_vec  5 dwconv_bwd_t_odd
 *       6 dwconv_bwd_t_generic;  7 refused — the entry point answers SPH3D_EUNSUPPORTED (a two-input shape that is not covered;
 *       deterministic mode and a shape only dwconv_bwd_t_generic's float atomics serve) and every other field is 0
 *     1 R (depth multiplier)   2 LPE (fwd_multi: lanes per edge, 16 for C <= 64, else 32)   3 V (bwd_vec: channels per lane, 4 or 2;
 *     bwd_odd: T, 1 .. 4)   4 MAXF (bwd_vec, bwd_odd: bin rows of the instantiation, 33 or 65)   5 PARTS (bwd_vec: 1 full, 2 half, 4
 *     quarter waves take alternate in-edges; bwd_odd: 1)   6 nslices (channel slices)   7 compact_launch (bwd_vec: the compact
 *     table's sweep is launched in front of the full one; the device chooses which of them works)   8 hub (bwd_vec: the sweeps
 *     leave hub sources to a hub launch behind each)   9 hub_threshold (in-edges above which a source is a hub; 0 without hubs)
 *     10 11 12 the full table: parts (position ranges per cloud), W (workgroups per XCD and slice), slabs (8 W)
 *     13 14 15 the compact table (bwd_vec)   16 reduce_slabs, 17 reduce_slabs_compact (the slab counts reduce_filter_partials is told
 *     for a full and for a compact run; 0: no reduce launch)   18 lds (dynamic LDS bytes of the main launch)   19 grid (its
 *     workgroups: fwd_*, bwd_generic, the full table's sweep)   20 hub_list_offset (bwd_vec: bytes from the workspace's start)
 *     21 workspace_bytes (gradient: sph3d_depthwise_conv3d_grad_t_workspace() for the shape, which asks with M = 0)
 *   The forward takes the first of multi, row, generic whose shape conditions hold and whose filter table fits 160 KiB of LDS.
 * -> SPH3D_OK (also for kernel 7), or SPH3D_EINVAL for an unknown op, a flag outside the above, Cb != 0 with a one-input op,
 *    out == NULL, or dimensions the entry point itself rejects. */
#define SPH3D_CONV_FWD 0
#define SPH3D_CONV_FWD_CAT 1
#define SPH3D_CONV_GRAD_T 2
#define SPH3D_CONV_GRAD_T_CAT 3
#define SPH3D_CONV_PLAN_FIELDS 22
int sph3d_depthwise_conv3d_plan(int op, int B, int N, int M, int F, int Ca, int Cb, int r, int K, int deterministic, int active_given,
                                long long* out);

/* ---- the training loop's optimiser update (train_s3dis.py:224, tf.train.AdamOptimizer) over flat fp32 buffers: one streaming
 * pass, torch.optim.Adam's arithmetic (no amsgrad / weight decay); step = 1, 2, ... (bias corrections are computed on the host) */
int sph3d_adam_step(long long n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                    float beta2, float eps, int step, sph3d_stream_t stream);

/* ---- the reference's own optimiser forms (train_s3dis.py:223-226: tf.train.AdamOptimizer(lr, epsilon=1e-4) or
 * tf.train.MomentumOptimizer(lr, momentum, use_nesterov=True)) over flat fp32 buffers of n elements: one streaming pass, 16-byte
 * lanes where every pointer is 16-byte aligned, scalar lanes otherwise.  With g = grad_scale * grad (grad_scale: 1 / world size
 * when a mean loss is sharded over ranks), every operation rounded once:
 *   rule 0, TensorFlow's Adam (slot0 = m, slot1 = v):  m += (1 - b1)(g - m);  v += (1 - b2)(g g - v);
 *           p -= (lr_t m) / (sqrt(v) + eps),  lr_t = lr sqrt(1 - b2^step) / (1 - b1^step) computed here in double and rounded
 *           once; step = 1 for the first update.  (sph3d_adam_step is torch's form, eps outside the bias correction.)
 *   rule 1, TensorFlow's Nesterov momentum (slot0 = accum, slot1 may be NULL; beta2, eps are not read):
 *           accum = momentum accum + g;  p -= g lr + (accum momentum) lr.
 * nonfinite (device, nullable): += the number of elements whose g is not finite; those elements are updated as written.
 * n == 0 is a no-op; SPH3D_EINVAL: a rule outside {0, 1}, step < 1, n < 0, a null buffer with n > 0. */
int sph3d_train_update(long long n, float* param, const float* grad, float* slot0, float* slot1, int rule, float lr,
                       float beta1_or_momentum, float beta2, float eps, int step, float grad_scale, long long* nonfinite,
                       sph3d_stream_t stream);

/* ---- the guarded update: clip by the global norm, skip a step whose gradient is not finite, keep an averaged copy of the
 * weights — decided on the device and consumed there, no host read (harness/guard.py is the statement, bit for bit).  Three
 * launches on `stream`: the sum of squares, the decision, the update.  With gg0_i = fl32(grad_scale grad_i):
 *   bad  = #{i : gg0_i not finite};   S = sum of (double)gg0_i^2 in ONE fixed order (2^18 lanes, lane l adds the elements
 *          i = l mod 2^18 in ascending i from +0.0, the lanes are reduced by the adjacent-pair tree), norm = sqrt(S) in double:
 *          the same bits whatever the pointers' alignment; a NaN's payload is the one thing left open;
 *   skip = skip_nonfinite && bad > 0: skipped += 1, nonfinite += bad, and param, the slots, ema and the powers keep their bits;
 *   else   applied += 1; rule 0: b1pow *= (double)beta1, b2pow *= (double)beta2, lr_t = fl32(lr sqrt(1 - b2pow) / (1 - b1pow))
 *          (running powers: lr_t is a function of the APPLIED count, which the host cannot know; sph3d_train_update's `step` has
 *          no counterpart here); rule 1: lr_t = lr;
 *          c = clip_norm / (norm + 1e-6) in double; clipped = clip_norm > 0 && bad == 0 && c < 1; c32 = fl32(c) when
 *          clip_norm > 0 && bad == 0, else 1; gg_i = fl32(c32 gg0_i) when clipped, else gg0_i; sph3d_train_update's rule 0 or 1
 *          on gg, operation for operation (with bad > 0 and no skip the NaN propagates as there, nonfinite += bad);
 *          ema (nullable: no average): d = min(ema_decay, (1 + a) / (10 + a)) with a = the updates applied before this one
 *          (tf.train.ExponentialMovingAverage(decay, num_updates)), om = fl32(1 - d), ema_i -= fl32(fl32(ema_i - param'_i) om).
 * state: SPH3D_GUARD_STATE_WORDS 8-byte words on the device, carried from step to step; the caller creates it with every word 0
 * except b1pow = b2pow = 1.0 and flag = 1.  Words (d: double, u: unsigned 64-bit; the three fp32 scalars are kept as doubles):
 *    0 d S              1 u bad (this step)   2 u applied          3 u skipped        4 u clipped_steps
 *    5 d b1pow          6 d b2pow             7 d last_norm        8 d max_norm_seen (a NaN norm never replaces it)
 *    9 d lr_t          10 d c32              11 d om              12 u flag: 0 skipped, 1 applied, 3 applied and clipped
 *   13..15 reserved (0).   Words 7..11 are those of the last APPLIED step; a skipped step writes words 0, 1, 3 and 12 only.
 * workspace: sph3d_train_guard_workspace(n) bytes, 8-byte aligned, the caller's (no entry allocates); dead when the call's
 * kernels are done.  n == 0 is a no-op.  SPH3D_EINVAL: a rule outside {0, 1}, n < 0, a null buffer with n > 0, ema with an
 * ema_decay outside (0, 1), a NaN clip_norm; SPH3D_EWORKSPACE: a null, short or misaligned workspace. */
#define SPH3D_GUARD_STATE_WORDS 16
size_t sph3d_train_guard_workspace(long long n);
int sph3d_train_update_guarded(long long n, float* param, const float* grad, float* slot0, float* slot1, float* ema, int rule, float lr,
                               float beta1_or_momentum, float beta2, float eps, float grad_scale, float clip_norm, int skip_nonfinite,
                               float ema_decay, long long* state, long long* nonfinite, void* workspace, size_t workspace_bytes,
                               sph3d_stream_t stream);
/* dst[0..n) = src[0..n) (fp32) if the state's last decision was a skip (flag == 0); otherwise nothing is written.  What a step
 * wrote before the decision existed (the batch-norm moving statistics) is put back this way from a copy taken before it. */
int sph3d_guard_restore(long long n, float* dst, const float* src, const long long* state, sph3d_stream_t stream);

/* ---- the reference's per-step training metrics and its one-pass validation counts (train_s3dis.py:371-376, :461-474) on the
 * device, without the copy of the logits to the host.  logits [B,N,C] fp32, label [B,N] int32, inner [B,N] int32 or NULL (every
 * row counts: the ShapeNet, RueMonge and ModelNet lines; ModelNet with N = 1).  For every counted row (inner > 0): with the
 * label outside [0, C) counters[2] += 1 and nothing else; otherwise pred = the first maximum of the row's C logits (a NaN counts
 * as a maximum, as np.argmax and sph3d_vote_finalize), confusion[label * C + pred] += 1, counters[0] (seen) += 1, counters[1]
 * (correct) += pred == label, counters[3] += 1 if a logit of the row is not finite.  counters[4] += 1 per call.  loss_sum[0]
 * (double) += the loss_parts fp32 values at loss_part, added in index order in float64 by one thread (loss_part may be NULL).
 * confusion [C*C] and counters [5] are int64; everything is accumulated, nothing zeroed, no floating-point atomic is used and the
 * result is a pure function of the inputs and the order of the calls.  C <= 64 (SPH3D_EUNSUPPORTED above). */
int sph3d_train_metrics(int B, int N, int C, const float* logits, const int* label, const int* inner, const float* loss_part,
                        int loss_parts, long long* confusion, long long* counters, double* loss_sum, sph3d_stream_t stream);

/* ---- keyed inverted dropout (the classifiers' tf.layers.dropout) as a pure function of its arguments: no generator state, so a
 * resumed run drops what the uninterrupted one drops.  x, y [B, row_len] fp32 (y may be x).  Element i of row b is kept iff the
 * high word of feed_draw(feed_cloud_key(seed, step, row0 + b), 16 + layer, i) (csrc/feed_draws.hpp) is >= threshold, and then
 * y = x * scale; a dropped element is +0.0 whatever x holds (inf, NaN).  The caller computes threshold = min(2^32 - 1,
 * ceil(rate * 2^32)) and scale = (float)(1 / (1 - rate)); the gradient is the same call on grad_output.  harness/dropout.py states
 * the op in numpy; the device result equals it bit for bit.  SPH3D_EINVAL: row_len >= 2^32, a layer outside [0, 16), row0 < 0 or
 * row0 + B > 2^32. */
int sph3d_dropout_keyed(int B, long long row_len, const float* x, float* y, unsigned long long seed, unsigned long long step,
                        long long row0, int layer, unsigned int threshold, float scale, sph3d_stream_t stream);

/* ---- the input side of the S3DIS training loop (train_s3dis.py:114-142,343-347) on the device: one launch assembles a batch
 * from a resident pool of parsed blocks.  rows [T,8] fp32: all blocks back to back, a row = xyz, rgb, label, inner (what
 * parse_fn builds); offsets [P+1] int64; block_ids [B] int32 (device): the blocks of this batch in batch order.  Per cloud b
 * with n rows: n >= num_point -> num_point DISTINCT rows in random order (a keyed bijection, cycle-walked), else num_point rows
 * with replacement.  augment = 1: clouds [0, B/3) are turned about z by a uniform angle and then by the small random rotation,
 * clouds [B/3, 2(B/3)) get clipped normal noise on xyz; colours, labels and the rest pass through.  Every draw is a pure
 * function of (seed, step, b, slot, purpose): no generator state, the same batch on any rank (csrc/feed.hip states the draws).
 * -> points [B,num_point,6] fp32, label / inner [B,num_point] int32, index [B,num_point] int32 (nullable): the row of its block
 * each point came from.  A block id outside [0, P) or an offset pair outside [0, T] reads nothing: zeros and index -1. */
int sph3d_feed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                        const int* block_ids, unsigned long long seed, unsigned long long step, int augment, float* points,
                        int* label, int* inner, int* index, sph3d_stream_t stream);

/* ---- training crops drawn from whole scenes on the device: one launch cuts a batch of B crops out of a resident pool of
 * column-sorted scenes (harness/cropfeed.py states the pool and the draws in numpy; csrc/cropfeed.hip).  A scene's rows are sorted
 * by the column col = ix n_y + iy of an xy grid of n_x x n_y cells (ties in original order), so the rows of cells (ix, y0 .. y1)
 * are one contiguous range.  The pool, all on the device:
 *   rows [T,8] fp32       the scenes' sorted rows back to back: xyz, rgb, label, a column that is not read (16-byte aligned)
 *   column [T] int32      the column of every row
 *   col_start [C] int32   per scene n_x n_y + 1 words: the first row (within the scene) of every column, then n
 *   scene_tab [S,5] int64 per scene: its first row in rows, its first word in col_start, n_x, n_y, n
 * scene_ids [B] int32 (device): the scene of every cloud.  Per cloud b, ck its key (csrc/feed_draws.hpp): attempt a < attempts
 * centres a window on the column (cx, cy) of row mulhi(hi32(draw(ck, 40, a)), n): ix in [max(0, cx - outer_half),
 * min(n_x - 1, cx + outer_half)], iy likewise; its members are the rows of its strips in ascending ix, then in stored order, T_a of
 * them.  The first attempt with T_a >= min_points is taken, else the one with the largest T_a (the lowest a on a tie).  With T
 * members, slot j takes member sph3d_feed_assemble's sample of (ck, T, num_point) names; inner = 1 iff the row's cell is within
 * inner_half of (cx, cy) on both axes; `augment` is sph3d_feed_assemble's rule by thirds of B.
 * -> points [B,num_point,6] fp32, label / inner [B,num_point] int32, index [B,num_point] int32 (nullable): the row within the
 * scene's stored order, crop [B,4] int32: scene id, centre row, attempt, T.  A scene id outside [0, S) or a scene_tab row that does
 * not describe rows of the pool reads nothing: zeros, index -1, crop -1.  Integer outputs are pure functions of the arguments; no
 * atomics, no workspace.  SPH3D_EINVAL: null or misaligned pointers, B num_point > 2^31 - 1, B > 65535, 2 outer_half + 1 > 256,
 * inner_half outside [0, outer_half], attempts outside [1, 8], min_points < 1. */
int sph3d_cropfeed_assemble(int B, int num_point, int num_scenes, long long total_rows, long long total_cols, const float* rows,
                            const int* column, const int* col_start, const long long* scene_tab, const int* scene_ids,
                            unsigned long long seed, unsigned long long step, int augment, int inner_half, int outer_half,
                            int attempts, int min_points, float* points, int* label, int* inner, int* index, int* crop,
                            sph3d_stream_t stream);

/* ---- overlap-voting evaluation of the segmentation nets on the device (s3dis_seg/evaluate_s3dis_with_overlap.py:253-286 the
 * per-pass sample counts and coverage, :301-302 the vote, :314-325 arg-max and the per-class counts; the ScanNet script,
 * evaluate_scannet_withoverlap.py:280, differs in the coverage threshold).  A batch is B blocks of the pool sph3d_feed_assemble
 * reads (rows [T,8], offsets [P+1], block_ids [B], all on the device) whose rows lie inside the pool rows
 * [row_base, row_base + batch_rows); votes [batch_rows, C] fp32, count / pred [batch_rows] int32 and the workspace's stamps are
 * indexed by (pool row - row_base); covered / inner_size [B] int32; remaining [1] int32.  The block ids of a batch are distinct.
 * A block id outside [0, P), or a block that is not inside that range, takes no part: it votes nothing and its inner_size is 0.
 * Every buffer is the caller's (the workspace holds sph3d_vote_workspace(batch_rows) bytes, 8-byte aligned, and belongs to the
 * batch from begin to the last accumulate); nothing is allocated, no floating-point atomic is used, and every output is a pure
 * function of the inputs (harness/evalvote.py:vote_reference states it in numpy, bit for bit, the fp32 sums included).
 *   begin       zeroes votes, count, covered and the stamps; inner_size[b] = rows of block b with inner == 1;
 *               remaining = blocks with inner_size > 0.
 *   accumulate  one pass: index [B,num_point] (what sph3d_feed_assemble returned; -1 or a row outside its block votes nothing),
 *               logits [B,num_point,C] fp32.  numpy's `sum[index] += logits` keeps the LAST of several slots that drew the same
 *               row; so does this: per pass a drawn row gets one logits vector added to its sums and one count.  An inner row
 *               whose count reaches min_votes adds one to covered[b]; remaining = blocks with covered < inner_size.
 *               pass = 0, 1, ... must increase from call to call within a batch (it orders the stamps), pass < 2^20.
 *   finalize    pred[row] = first maximum of the row's C sums (a NaN counts as a maximum, as np.argmax); for inner rows with a
 *               label in [0, C): confusion[label * C + pred] += 1 (int64, accumulated, not zeroed here); *nonfinite += rows of
 *               the batch's blocks whose sums are not all finite.  C <= 64. */
size_t sph3d_vote_workspace(long long batch_rows);
int sph3d_vote_begin(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                     const int* block_ids, long long row_base, long long batch_rows, float* votes, int* count, int* covered,
                     int* inner_size, int* remaining, void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_vote_accumulate(int B, int num_point, int C, int num_blocks, long long total_rows, const float* rows,
                          const long long* offsets, const int* block_ids, long long row_base, long long batch_rows, int pass,
                          const int* index, const float* logits, int min_votes, float* votes, int* count, int* covered,
                          const int* inner_size, int* remaining, void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_vote_finalize(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                        const int* block_ids, long long row_base, long long batch_rows, const float* votes, int* pred,
                        long long* confusion, long long* nonfinite, sph3d_stream_t stream);

/* ---- the input side of the object datasets (shapenet_seg/train_shapenet.py:121-152, modelnet40_cls/train_modelnet.py:95-115,
 * shapenet_seg/evaluate_shapenet.py:86-94) on the device: one launch assembles a batch from a resident pool of shapes.  The pool
 * is sph3d_feed_assemble's (rows [T,8]: xyz in columns 0:3, the label in column 6; offsets [P+1]; shape_ids [B] int32, device),
 * and so are the sample draws: index is the same pure function of (seed, step, b, n, num_point) and does not depend on recipe.
 * recipe [B] int32 (device): per cloud a bit mask, applied in the reference's order (utils/data_util.py) —
 *   1 TURN   xyz . Rz(2 pi u);   2 TILT   . Rz Ry Rx of three normal angles (sigma 0.06, clipped at 0.18);
 *   4 SCALE  * (0.8 + 0.45 u);   8 SHIFT  + (-0.1 + 0.2 u) per axis;   16 JITTER  + normal noise per point (sigma 0.01, clip 0.02);
 * bits above 16 are ignored.  A mask of 0 copies xyz bit for bit.  Every draw is a pure function of (seed, step, b, slot, purpose)
 * (csrc/feed_draws.hpp, csrc/objfeed.hip; harness/objfeed.py states them in numpy).
 * -> points [B,num_point,3] fp32, label [B,num_point] int32, index [B,num_point] int32 (nullable): the row of its shape each
 * point came from.  A shape id outside [0, P) or an offset pair outside [0, T] reads nothing: zeros and index -1.  B <= 65535. */
int sph3d_objfeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                           const int* shape_ids, unsigned long long seed, unsigned long long step, const int* recipe,
                           float* points, int* label, int* index, sph3d_stream_t stream);

/* ---- the input side of the ScanNet line (scannet_seg/train_scannet.py:112-127, evaluate_scannet_withoverlap.py:94-116,282-286)
 * on the device: one launch assembles ALL views of one draw from a resident pool of blocks.  The pool is sph3d_feed_assemble's
 * (rows [T,8]: xyz, rgb, label, inner; offsets [P+1]; block_ids [B] int32, device), and so are the sample draws: index, label and
 * inner are the same pure function of (seed, step, b, n, num_point), whatever the recipes, and equal what
 * sph3d_feed_assemble(..., augment = 0) writes bit for bit.  recipe [views,B] int32 (device): the bit masks, purposes and
 * counters of sph3d_objfeed_assemble.  View v's xyz is recipe[v][b] applied to the fp32 xyz of view v - 1 (view -1: the pool
 * row) — the reference augments its float32 batch in place, view after view — with its transform draws taken from
 * feed_view_key(ck, v) (csrc/feed_draws.hpp): view 0's key is the cloud's own, so a one-view launch draws exactly what
 * sph3d_objfeed_assemble draws; view v >= 1 uses one more splitmix round over (ck, v).  A mask of 0 copies the previous view bit
 * for bit; rgb is copied into every view (csrc/scanfeed.hip; harness/scannet.py states it in numpy).
 * -> points [views,B,num_point,6] fp32 (8-byte aligned); label, inner [B,num_point] int32; index [B,num_point] int32 (nullable).
 * A block id outside [0, P) or an offset pair outside [0, T] reads nothing: zeros in every view, label 0, inner 0, index -1.
 * 1 <= views <= 4, B <= 65535, views * B * num_point <= 2^31 - 1. */
int sph3d_blockfeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                             const int* block_ids, unsigned long long seed, unsigned long long step, int views, const int* recipe,
                             float* points, int* label, int* inner, int* index, sph3d_stream_t stream);

/* ---- the input side of the RueMonge2014 facade line (ruemonge2014_seg/train_ruemonge2014.py:98-138,159,
 * ruemonge2014_seg/evaluate_ruemonge2014.py:180-305, utils/data_util.py:64-105; records: io/make_tfrecord_ruemonge2014.py:45-57) on
 * the device: one launch assembles a batch of 9-channel clouds from a resident pool of facade splits.  The pool is
 * sph3d_feed_assemble's (rows [T,8]: xyz, rgb, label, inner; offsets [P+1]; ids [B] int32, device) plus normals [T,4] fp32
 * (nx, ny, nz and a padding column that is never written out; 16-byte aligned).  The sample draws are sph3d_feed_assemble's: index
 * is the same pure function of (seed, step, b, n, num_point) and does not depend on recipe.  recipe [B] int32 (device): the bit
 * masks, purposes and counters of sph3d_objfeed_assemble; TURN and TILT multiply xyz AND the normal by the same matrix entries,
 * SCALE, SHIFT and JITTER touch xyz only, rgb and the label are always copied.  A mask of 0 copies all nine channels bit for bit;
 * a mask without TURN and TILT copies the normal bit for bit (csrc/facadefeed.hip; harness/facadefeed.py states it in numpy).
 * -> points [B,num_point,9] fp32 in the reference's channel order xyz, normal, rgb; label [B,num_point] int32; index
 * [B,num_point] int32 (nullable).  An id outside [0, P) or an offset pair outside [0, T] reads nothing: zeros in all nine
 * channels, label 0 and index -1.  B <= 65535, B * num_point <= 2^31 - 1. */
int sph3d_facadefeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows, const float* normals,
                              const long long* offsets, const int* ids, unsigned long long seed, unsigned long long step,
                              const int* recipe, float* points, int* label, int* index, sph3d_stream_t stream);

/* ---- the per-shape part IoU counts of the ShapeNet evaluation (shapenet_seg/evaluate_shapenet.py:262-289,
 * evaluate_shapenet_onehot.py:283-314; csrc/shapeeval.hip): the finalize of a batch of sph3d_vote_* whose blocks are shapes (same
 * rows / offsets / shape_ids / row_base / batch_rows, votes [batch_rows, C] as the accumulates left them, the part label in
 * column 6 of the rows).  part_lo, part_n [B] int32 (device): the part range of each shape inside the C sums
 * (0 < part_n, part_lo + part_n <= C <= 64; a per-category model has part_lo = 0, part_n = C).
 *   pred[row] = part_lo[b] + first maximum of votes[row, part_lo[b] : part_lo[b] + part_n[b]] (a NaN counts as a maximum, as
 *   np.argmax); per shape b and part l of its range: inter[b*C + l] = rows with pred == l and label == l, pred_cnt[b*C + l] = rows
 *   with pred == l, gt_cnt[b*C + l] = rows with label == l; correct[b] = rows with pred == label.  A label outside the shape's
 *   range matches no part.  inter / pred_cnt / gt_cnt [B,C] and correct [B] int32 are zeroed here; *nonfinite (int64) += rows of
 *   the batch's shapes whose C sums are not all finite (accumulated, not zeroed).
 * A shape id outside [0, P), a shape that is not inside the batch's row range, or one whose part range is not inside [0, C)
 * takes no part: it counts nothing and none of its predictions is written.  Every buffer is the caller's; nothing is allocated,
 * no floating-point atomic is used; harness/shapeeval.py:shape_vote_reference states it in numpy. */
int sph3d_shape_iou(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                    const int* shape_ids, long long row_base, long long batch_rows, const float* votes, const int* part_lo,
                    const int* part_n, int* pred, int* inter, int* pred_cnt, int* gt_cnt, int* correct, long long* nonfinite,
                    sph3d_stream_t stream);

/* ---- the ModelNet40 classification evaluation on the device (modelnet40_cls/evaluate_modelnet.py:149-223; csrc/clseval.hip;
 * harness/clseval.py states every entry in numpy).  Every buffer is the caller's; nothing is allocated, no floating-point atomic
 * is used, and every id and label is checked against its range before an address is formed.
 *   clsfeed_assemble     the whole-shape batch: sph3d_objfeed_assemble's pool, draws, purposes and counters (csrc/feed_draws.hpp),
 *                        without the label output and with two more arguments.  order = 1: slot i reads row i of its shape — the
 *                        stored order the reference evaluates in (evaluate_modelnet.py:170-177; farthest-point sampling starts from
 *                        row 0) —, slots i >= n write zeros and index -1; order = 0: the feed's draw.  swap_yz = 1 exchanges
 *                        columns 1 and 2 of the row before any transform: `batch_xyz[:, :, [0, 2, 1]]` of evaluate_modelnet.py:173
 *                        and train_modelnet.py:278,337.  recipe [B] int32 (device): bits 1 TURN, 2 TILT, 4 SCALE, 8 SHIFT
 *                        (evaluate_modelnet.py:71-78, train_modelnet.py:104-113; utils/data_util.py:47-61,140-204); the kernel reads
 *                        no other bit, and the binding refuses a mask above 15 before it uploads it.  A mask of 0 copies bit for
 *                        bit.  -> points [B,num_point,3] fp32, index [B,num_point] int32 (nullable).  A shape id outside [0, P) or
 *                        an offset pair outside [0, T] reads nothing: zeros and index -1.  B <= 65535, B * num_point <= 2^31 - 1.
 *   cls_vote_accumulate  `batch_pred_sum += pred_val` of evaluate_modelnet.py:180,196 in float64: sums[b,c] = 0.0 + (double)
 *                        logits[b,c] for vote 0 (the sum starts from np.zeros, so a logit of -0.0 leaves +0.0), sums[b,c] +=
 *                        (double)logits[b,c] for the votes after it — one float64 add per vote, in vote order.  With votes_out
 *                        [P,num_votes,C] fp32 (nullable) the logits are also stored at [shape_ids[b], vote, :], the `pred_votes`
 *                        of :194; a shape id outside [0, num_blocks) stores none.  0 <= vote < num_votes, C <= 64.
 *   cls_vote_finalize    evaluate_modelnet.py:198-207: pred[shape_ids[b]] = first maximum of sums[b, :] (a NaN counts as a
 *                        maximum, as np.argmax); with label = category[shape_ids[b]]: counters[0] (seen) += 1, class_seen[label]
 *                        += 1, counters[2] (nonfinite) += 1 if one of the C sums is a NaN or an infinity, and counters[1]
 *                        (correct) and class_correct[label] += 1 if pred == label.  A label outside [0, C) counts in counters[3]
 *                        (bad_label) only; a shape id outside [0, num_blocks) counts nothing and writes no prediction.
 *                        pred [P], counters [4], class_seen [C], class_correct [C] int32 are accumulated, not zeroed. */
int sph3d_clsfeed_assemble(int B, int num_point, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                           const int* shape_ids, unsigned long long seed, unsigned long long step, const int* recipe, int order,
                           int swap_yz, float* points, int* index, sph3d_stream_t stream);
int sph3d_cls_vote_accumulate(int B, int C, const float* logits, int vote, int num_votes, double* sums, const int* shape_ids,
                              float* votes_out, int num_blocks, sph3d_stream_t stream);
int sph3d_cls_vote_finalize(int B, int C, const double* sums, const int* shape_ids, const int* category, int num_blocks, int* pred,
                            int* counters, int* class_seen, int* class_correct, sph3d_stream_t stream);

/* ---- scene-level evaluation (post-merging/s3dis_merge.m:42-82, scannet_merge.m:28-55; csrc/scene.hip): the blocks' vote sums are
 * normalised per row, merged into a per-scene array through the records' index_label, and the arg-max is lifted to the
 * full-resolution cloud through a nearest-neighbour search.  harness/scenemerge.py states every entry in numpy, bit for bit, the
 * fp32 probabilities included.  Every buffer is the caller's; nothing is allocated and no floating-point atomic is used.
 *   scene_merge     the batch of sph3d_vote_* (same rows / offsets / block_ids / row_base / batch_rows, votes [batch_rows, C] as
 *                   the voter left them); index [T] int32: the pool rows' index_label.  Blocks are taken in the order of block_ids
 *                   (pass them ascending: the statement merges in pool order), one launch each.  Per INNER row: s = sum of v*v
 *                   (ascending c, separate fp32 multiply and add), r = sqrt(s), u = v / r, e = exp32(u) (include/sph3d_exp32.h),
 *                   z = sum of e, merged[index[row], c] += e_c / z and hits[index[row]] += 1.  A row with s == 0 or s not finite
 *                   adds nothing and counts in counters[0] (skipped_rows); then an index outside [0, V) counts in counters[1]
 *                   (out_of_scene).  merged [V, C] fp32, hits [V] int32 and counters [2] int64 are accumulated, not zeroed.
 *                   The inner indices of one block must be distinct (harness/feed.py refuses a pool where they are not).
 *   scene_finalize  pred_voxel[i] = first maximum of merged[i, :], 0 for a row with hits == 0, which counts in *unseen_rows;
 *                   with voxel_label [V] (nullable, together with confusion): confusion[label * C + pred] += 1 for labels in [0, C).
 *   nn1             idx[f] = the reference point that minimises the fp32 d2 = (dx*dx + dy*dy) + dz*dz, dx = q.x - r.x; ties go to
 *                   the lowest index; a d2 that is not finite never wins (so a reference point with a non-finite coordinate is
 *                   never chosen); -1 for a query with a non-finite coordinate or without any candidate.  ref_xyz [V, 3],
 *                   query_xyz [F, 3].  mode SPH3D_NN1_GRID: counting sort of the reference into a cell grid and an exact ring walk
 *                   per query, falling back to brute force on the device for clouds the grid cannot index (fewer than 64 finite
 *                   points, a non-finite or zero extent); SPH3D_NN1_BRUTE: tiled brute force.  Both give the same idx.
 *                   The workspace holds sph3d_nn1_workspace(V, F) bytes, 16-byte aligned.
 *   scene_lift      pred_full[f] = pred_voxel[idx[f]] (-1 where idx is outside [0, V)), mapped through label_map [C] when given
 *                   (ScanNet's labelid_set); with label_full [F] (nullable, together with confusion):
 *                   confusion[label * C + unmapped prediction] += 1 for labels in [0, C) and idx >= 0.
 * C <= 64; V, F < 2^31. */
#define SPH3D_NN1_GRID 0
#define SPH3D_NN1_BRUTE 1
int sph3d_scene_merge(int B, int C, int num_blocks, long long total_rows, const float* rows, const long long* offsets,
                      const int* index, const int* block_ids, long long row_base, long long batch_rows, const float* votes,
                      long long V, float* merged, int* hits, long long* counters, sph3d_stream_t stream);
int sph3d_scene_finalize(int C, long long V, const float* merged, const int* hits, const int* voxel_label, int* pred_voxel,
                         long long* unseen_rows, long long* confusion, sph3d_stream_t stream);
size_t sph3d_nn1_workspace(long long V, long long F);
int sph3d_nn1(long long V, long long F, const float* ref_xyz, const float* query_xyz, int mode, int* idx, void* workspace,
              size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_scene_lift(int C, long long V, long long F, const int* pred_voxel, const int* idx, const int* label_map,
                     const int* label_full, int* pred_full, long long* confusion, sph3d_stream_t stream);

/* ---- exact k nearest neighbours (csrc/knn.hip; not in the reference, whose searches are range searches that keep the FIRST
 * nn_sample points in index order).  harness/knn.py states it in numpy (knn_reference); nn_index, nn_count and the bit patterns of
 * nn_dist equal that statement at every launch form.  database [B,N,3], query [B,M,3] fp32 -> nn_index [B,M,k] int32,
 * nn_count [B,M] int32, nn_dist [B,M,k] fp32: the format of the range searches, so every consumer of theirs takes the graph.
 *   d2         dx = q.x - p.x (and y, z), d2 = (dx*dx + dy*dy) + dz*dz: fp32, one rounding per operation (sph3d_nn1's d2).
 *   admitted   a database point is a candidate of a query iff d2 is finite and d2 < R2, R2 = radius * radius in fp32.  radius = +inf
 *              is "no radius" (R2 = inf: every finite d2).  THIS PREDICATE IS THE OP'S OWN: it is not the reference kernel's
 *              fabs(dist - radius) > 1e-6 test, and no radius grows.
 *   row        the admitted candidates in ascending (d2, index) order — the lowest index first among equal d2 — cut at k.
 *              nn_count = min(k, admitted): 0 is possible with a radius, and for a query with a non-finite coordinate (a database
 *              point with one is never returned).  Unused slots hold index 0 and distance 0.
 *   nn_dist    SPH3D_KNN_DIST_ROOT: sqrt(sqrt(d2)), two correctly rounded fp32 roots — the library's convention (the square root
 *              of the Euclidean distance), so sph3d_spherical_kernel and the weighted un-pooling take the tensor as it is;
 *              SPH3D_KNN_DIST_SQUARED: d2 itself.
 *   mode       SPH3D_KNN_SCAN: every wave scans its cloud from LDS tiles; SPH3D_KNN_GRID: a counting-sorted cell grid per cloud in
 *              the caller's workspace (the layout of sph3d_nn1's) and a walk of cube shells per query; clouds the grid cannot index
 *              (fewer than 64 finite points, a zero or non-finite extent) raise a flag on the device and the scan, queued behind
 *              the search, takes them — the host reads nothing.  SPH3D_KNN_AUTO: the scan up to 2048 points, the grid above (the measured crossover).
 *              All three give the same output.
 * 1 <= k <= 64 (k > 64: SPH3D_EUNSUPPORTED; k < 1: SPH3D_EINVAL), then radius > 0 (not NaN), then B >= 0, N >= 1, M >= 0 with
 * B N <= 2^40 and B M <= 2^40, then mode and dist: validated in this order by the entry and by the plan query alike.  B == 0 or
 * M == 0 launches nothing.  workspace: sph3d_build_nearest_neighbor_workspace(B, N, M, k, mode) bytes, 16-byte aligned (0 for
 * the scan and for arguments the entry rejects); too small: SPH3D_EWORKSPACE.  Nothing is allocated.
 *
 * sph3d_build_nearest_neighbor_plan: what the call will launch (csrc/knn_plan.hpp: knn_plan, which the entry launches from and the
 * workspace query sizes from), answered on the host.  out[SPH3D_KNN_PLAN_FIELDS], in this order:
 *     0 form: SPH3D_KNN_FORM_NONE (B == 0 or M == 0), _SCAN, _GRID   1 queries per workgroup (one wave each)   2 block (threads)
 *     3 groups = ceil(M / queries) per cloud   4 scan_grid: workgroups of knn_scan_kernel, min(B groups, 2^20) (every kernel strides
 *     over its work items)   5 scan_lds: its static LDS bytes   6 search_grid, 7 search_lds: knn_grid_kernel (_GRID)
 *     8 fallback (_GRID: 1, knn_scan_kernel is queued behind the search and runs per cloud only where the build raised the flag)
 *     9 cells: cells a cloud's grid may have, N / 2 held to [64, cell_cap]   10 cell_cap = 2^21
 *     11 build_block, 12 build_parts (workgroups per cloud, at most 64), 13 build_grid: the bounding-box, count and fill passes
 *     14 setup_grid: header reset and grid shape, a thread per cloud   15 prefix_block, 16 prefix_grid: the scan of the cell counts
 *     17 workspace_bytes, the byte offsets into it: 18 headers, 19 cell ends, 20 sorted points (x, y, z, index bits), and the
 *     strides per cloud: 21 header (256), 22 cell ends, 23 points (16 N)
 * -> SPH3D_OK, or the entry's own status and message in the entry's order, then SPH3D_EINVAL for out == NULL. */
#define SPH3D_KNN_AUTO 0
#define SPH3D_KNN_SCAN 1
#define SPH3D_KNN_GRID 2
#define SPH3D_KNN_DIST_ROOT 0
#define SPH3D_KNN_DIST_SQUARED 1
#define SPH3D_KNN_FORM_NONE 0
#define SPH3D_KNN_FORM_SCAN 1
#define SPH3D_KNN_FORM_GRID 2
#define SPH3D_KNN_PLAN_FIELDS 24
size_t sph3d_build_nearest_neighbor_workspace(int B, int N, int M, int k, int mode);
int sph3d_build_nearest_neighbor_plan(int B, int N, int M, int k, float radius, int mode, long long* out);
int sph3d_build_nearest_neighbor(int B, int N, int M, int k, float radius, int mode, int dist, const float* database,
                                 const float* query, int* nn_index, int* nn_count, float* nn_dist, void* workspace,
                                 size_t workspace_bytes, sph3d_stream_t stream);

/* ---- surface normals from order-free integer ball moments (csrc/normals.hip; not in the reference, whose facade line reads its
 * normals from the dataset).  harness/normals.py states every entry in numpy: moments and counts equal it bit for bit, normal and
 * variation are held to the per-element bounds of tests/_normal_ref.py.  Every buffer is the caller's; no floating-point atomic.
 *   offsets     query q, neighbour p, both fp32 xyz: d_a = p_a - q_a (one fp32 subtraction per axis); Q = 262144.0 / (double)radius
 *               (one double division); t_a = rint((double)d_a * Q) (one double product, ties to even).  A neighbour is VALID when
 *               fabs((double)d_a) * Q <= 2^21 on all three axes, evaluated in double; a non-finite coordinate fails and the
 *               neighbour is skipped.  A query with a non-finite coordinate has no valid neighbour.
 *   moments     ten signed 64-bit integers per query over its valid neighbours: n; S1_x, S1_y, S1_z = sum t_a; S2_xx, S2_xy, S2_xz,
 *               S2_yy, S2_yz, S2_zz = sum t_a t_b.  |t| <= 2^21 and n < 2^16 (graph form) or |t| <= 2^18 and n <= 2^26 (ball form):
 *               nothing overflows, and integer sums do not depend on the order the neighbours are visited in.
 *   covariance  float64, every operation rounded once (no contraction): m_a = (double)S1_a / n, c_ab = (double)S2_ab / n - m_a m_b.
 *   normal      l0 <= l1 <= l2 the eigenvalues of c: the unit eigenvector of l0; variation = max(l0, 0) / (l0 + l1 + l2) as fp32.
 *               A row with n < min_count (min_count >= 3) or with a trace (c_xx + c_yy) + c_zz that is not positive gets the
 *               normal (0, 0, 0) and variation 0; any other row a unit vector (a collinear neighbourhood: some unit vector
 *               perpendicular to the line, and variation tells).
 *   sign        decided on the float64 vector before the rounding to fp32: first the component of largest magnitude is made
 *               positive (ties: the lowest axis); then, with `toward`, the normal is flipped when
 *               n . ((double)toward - (double)q) < 0; a product of exactly 0 keeps the canonical sign.
 *   graph_normals   database [B,N,3], query [B,M,3], nn_index [B,M,K], nn_count [B,M] as the searches leave them (compat or
 *               fixed radius mode, M != N, 0 < K < 2^16): the neighbours of a row are its first min(nn_count, K) entries, in list
 *               order; an entry outside [0, N) is skipped like an invalid one.  toward [B,3] or NULL.  -> normals [B,M,3];
 *               variation [B,M], count [B,M] int32 (= n), moments [B,M,10] int64, all three nullable; counters [1] int64
 *               (nullable): counters[0] += the skipped neighbours (accumulated, not zeroed).  No workspace.  B * M == 0: nothing
 *               is launched.
 *   ball_normals    xyz [V,3], a flat cloud (a facade, a room, a pool block), V <= 2^26.  The neighbours of a row are ALL rows
 *               with the fp32 predicate (dx*dx + dy*dy) + dz*dz < r2, dx = p.x - q.x, r2 = fp32(radius * radius), every operation
 *               rounded once as in nn1; the row itself is one of them.  toward [3] or NULL.  -> normals [V,3], count [V] int32,
 *               variation [V] and moments [V,10] nullable.  Walks nn1's counting-sorted cell grid, built with a cell edge of at
 *               least `radius`, and falls back to brute force on the device under nn1's conditions; both give the same moments.
 *               The workspace holds sph3d_ball_normals_workspace(V) bytes, 16-byte aligned.  V == 0: nothing is launched. */
int sph3d_graph_normals(int B, int N, int M, int K, float radius, int min_count, const float* database, const float* query,
                        const int* nn_index, const int* nn_count, const float* toward, float* normals, float* variation, int* count,
                        long long* moments, long long* counters, sph3d_stream_t stream);
size_t sph3d_ball_normals_workspace(long long V);
int sph3d_ball_normals(long long V, float radius, int min_count, const float* xyz, const float* toward, float* normals,
                       float* variation, int* count, long long* moments, void* workspace, size_t workspace_bytes,
                       sph3d_stream_t stream);

/* ---- scene preparation (MATLAB pcdownsample 'gridAverage', preprocesing/s3dis_prepare_data.m:35-37; the block writer,
 * io/make_tfrecord_s3dis.py:113-242; csrc/prep.hip): a full-resolution cloud is averaged over the cells of a grid, the voxel cloud
 * is recentred, and the blocks of a pool (rows [T,8], index [T], as sph3d_feed_assemble / sph3d_scene_merge read them) are cut
 * from it.  harness/sceneprep.py states every entry in numpy, bit for bit, the fp32 means included.  Every buffer is the
 * caller's; nothing is allocated, no floating-point atomic is used, every output is a pure function of the inputs.
 *   prep_voxel_grid      xyz [F,3], attr [F,A] fp32 (A <= 13; null for A = 0).  A point is KEPT when its 3+A values are finite and
 *                        at most 2^17 in magnitude.  lo / hi: extrema of the kept points; cell i_a = floor((v_a - lo_a) / h), both
 *                        operations rounded to fp32 once; n_a = i_a(hi_a) + 1; key = (i_x n_y + i_y) n_z + i_z; the voxel rows are
 *                        the occupied cells in ascending key.  -> voxel_of_point [F] int32 (-1: dropped) and header [16] int32 =
 *                        { V, dropped, flag, n_x, n_y, n_z, lo[3], hi[3] (fp32 bits), cells, 0, 0, 0 }, the one thing the host
 *                        reads before it allocates the [V, ...] arrays.  flag 1: the grid needs more than max_cells (<= 2^30) cells
 *                        (or an axis does); flag 2: no point is kept; with a flag V = 0, voxel_of_point is all -1 and no cell is
 *                        touched.  The workspace (sph3d_prep_voxel_grid_workspace(F, max_cells) bytes, 16-byte aligned) holds the
 *                        dense table, 4 bytes per cell of max_cells.
 *   prep_voxel_reduce    sums [V, 3+A] int64 and count [V] int32 (both zeroed here): sums[row, col] = sum over the row's points of
 *                        rint(v * 2^20) (the double product is exact; ties to even; wraps modulo 2^64), count = the row's points.
 *                        SPH3D_PREP_REDUCE_ATOMIC: 64-bit integer atomics, no workspace; SPH3D_PREP_REDUCE_SORTED: a counting
 *                        sort of the points by row and a per-row sum, workspace sph3d_prep_voxel_reduce_workspace(F, V, mode).
 *                        Integer sums: both give the same bits in any order.
 *   prep_voxel_finalize  voxel_xyz [V,3], voxel_attr [V,A] = f32(f64(sum) / f64(count) * 2^-20); box: as prep_box of voxel_xyz.
 *   prep_box             box [8] int32 = { lo[3], hi[3] of the finite points as ORDERED integers (an fp32 bit pattern u maps to
 *                        ~u when its sign bit is set, else u | 2^31), their count, 0 }.
 *   prep_normalise       make_tfrecord_s3dis.py:114-122 in fp32, each operation rounded once: c = (lo + hi) / 2 with c_z = lo_z
 *                        from `box`, out_xyz = xyz - c, out_rgb = (2 rgb) / 255 - 1.
 *   prep_rect_count      counts [R] int32 (zeroed here) = the points of xyz [V,3] with x_lo <= x <= x_hi and y_lo <= y <= y_hi for
 *                        each of rects [R,4] fp32 = (x_lo, x_hi, y_lo, y_hi), 16-byte aligned: all candidates of a scene in one call.
 *   prep_block_fill      rects [P,8]: per block the context-padded rectangle, then the plain one.  Block p receives the points
 *                        inside its padded rectangle in ASCENDING point index at rows [offsets[p], offsets[p+1]) of rows [T,8]
 *                        (xyz, rgb, (float)label, inner = inside the plain rectangle; 16-byte aligned) and index [T] (the point's
 *                        number); offsets [P+1] int64 come from prep_rect_count's counts of the padded rectangles.  A block whose
 *                        points are not as many as its range counts in *mismatch (accumulated) and nothing is written outside
 *                        its range.  Workspace: sph3d_prep_block_fill_workspace(V, P) bytes, 16-byte aligned. */
#define SPH3D_PREP_REDUCE_ATOMIC 0
#define SPH3D_PREP_REDUCE_SORTED 1
size_t sph3d_prep_voxel_grid_workspace(long long F, long long max_cells);
int sph3d_prep_voxel_grid(long long F, int A, const float* xyz, const float* attr, float h, long long max_cells,
                          int* voxel_of_point, int* header, void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
size_t sph3d_prep_voxel_reduce_workspace(long long F, long long V, int mode);
int sph3d_prep_voxel_reduce(long long F, int A, long long V, const float* xyz, const float* attr, const int* voxel_of_point,
                            int mode, long long* sums, int* count, void* workspace, size_t workspace_bytes, sph3d_stream_t stream);
int sph3d_prep_voxel_finalize(long long V, int A, const long long* sums, const int* count, float* voxel_xyz, float* voxel_attr,
                              int* box, sph3d_stream_t stream);
int sph3d_prep_box(long long V, const float* xyz, int* box, sph3d_stream_t stream);
int sph3d_prep_normalise(long long V, const float* voxel_xyz, const float* voxel_rgb, const int* box, float* out_xyz,
                         float* out_rgb, sph3d_stream_t stream);
int sph3d_prep_rect_count(long long V, int R, const float* xyz, const float* rects, int* counts, sph3d_stream_t stream);
size_t sph3d_prep_block_fill_workspace(long long V, int P);
int sph3d_prep_block_fill(long long V, int P, long long T, const float* xyz, const float* rgb, const int* label,
                          const float* rects, const long long* offsets, float* rows, int* index, int* mismatch, void* workspace,
                          size_t workspace_bytes, sph3d_stream_t stream);

/* the segmentation nets' training loss (models/SPH3D_s3dis.py:116-133: per block the mean over the points with inner_label > 0
 * of the sparse softmax cross-entropy, summed over the batch by the caller) and its gradient in one launch:
 *   loss_part[b * S + s], S = sph3d_masked_softmax_xent_parts(N): the shares of S slices of block b's points in
 *       loss_b = mean_{n: inner > 0} ( logsumexp(logits[b,n,:]) - logits[b,n,label[b,n]] )      (0 for a block without such points)
 *   dlogits[b,n,:] = d(sum_b loss_b) / d logits[b,n,:]
 * logits [B,N,C] fp32, label [B,N] int64, inner_label [B,N] fp32; deterministic (fixed-order reductions).
 * dlogits == NULL: the losses only (evaluation: no gradient pass, no [B,N,C] store).  An inner point whose label lies
 * outside [0, C) makes its block's loss and its gradient row NaN (the reference's GPU op yields NaN there as well). */
int sph3d_masked_softmax_xent_parts(int N);
int sph3d_masked_softmax_xent(int B, int N, int C, const float* logits, const long long* label, const float* inner_label,
                              float* loss_part, float* dlogits, sph3d_stream_t stream);

/* the Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) of every block and its gradient with respect to the logits
 * (csrc/lovasz.hip; the float64 statement is harness/lovasz.py: lovasz_reference).  It is not an op of the reference tree.
 * logits [B,N,C] fp32, label [B,N] int64, inner [B,N] fp32 or NULL (every row).  Per block b:
 *   valid   row n is valid iff (inner == NULL or inner[b,n] > 0; NaN > 0 is false) and label[b,n] != ignore; n_b valid rows
 *   probs   p = softmax(logits[b,n,:]) (maximum, expf, a sum in ascending c, a division), written for EVERY row
 *   class   for a class c with G = #{valid n: label = c} > 0 (a "present" class): e_n = 1 - p[n,c] on the valid rows labelled c
 *           (foreground), p[n,c] on the other valid rows; the valid rows in the order of DESCENDING e, ties by ASCENDING n (e is
 *           one fp32 operation on probs, so the order is an integer function of the probs written: bits(e) descending, n ascending);
 *           F_j foreground rows among the sorted positions 0..j, U_j = G + (j + 1) - F_j; the Lovasz gradient of the Jaccard loss
 *               g_j = 1 / U_j on a foreground position,   (G - F_j) / (U_j (U_j - 1)) on a background position
 *           (the paper's jaccard_j - jaccard_{j-1} with jaccard_j = (j + 1) / U_j, written without the cancellation; g >= 0 and
 *           sum_j g_j = 1);  class_loss[b,c] = sum_j e_(j) g_j, and 0 for a class that is not present
 *   loss    P_b present classes; loss[b] = (sum over c, ascending, of class_loss[b,c]) / P_b; 0 if P_b = 0
 *   coef    coef[b,n,c] = d loss[b] / d p[n,c] = -g_rank(n) / P_b on foreground, +g_rank(n) / P_b on background; 0 on rows that are
 *           not valid and for classes that are not present
 *   dlogits dlogits[b,n,k] = p_k (coef_k - sum_c coef_c p_c), zeros on rows that are not valid.  dlogits == NULL: no gradient pass
 *           (loss is produced all the same, with the same bits)
 *   order   order[b,c,j], [B,C,N] int32: the row at sorted position j of class c (present or not), -1 for j >= n_b.  NULL: not written
 * A valid row whose label lies outside [0, C), or whose probabilities are not finite, makes loss[b] and every dlogits row of block
 * b NaN (class_loss and coef of that block are then unspecified); nothing is clamped and every read stays in range.
 * probs and coef are workspaces the caller owns ([B,N,C] each); every reduction runs in a fixed order: the same inputs give the
 * same bits, deterministic mode or not.  Three launches; no workspace beyond the arguments.
 * N <= 16384 and C <= 1024 (the sort holds a block's keys in LDS): sph3d_lovasz_softmax_supported(N, C) -> 1 | 0 on the host.
 * -> SPH3D_OK; SPH3D_EINVAL for B < 0, N <= 0, C <= 0, B N C > 2^40, B C >= 2^31, B >= 2^16 or a null pointer other than
 * inner, dlogits and order; SPH3D_EUNSUPPORTED, before any launch and before the pointers are looked at, outside the shapes above. */
int sph3d_lovasz_softmax_supported(int N, int C);
int sph3d_lovasz_softmax(int B, int N, int C, const float* logits, const long long* label, const float* inner, long long ignore,
                         float* probs, float* coef, float* class_loss, float* loss, float* dlogits, int* order,
                         sph3d_stream_t stream);

/* the same loss for blocks of up to 2^20 rows: the sort runs in global memory (csrc/lovasz.hip; the host's choices are
 * csrc/lovasz_plan.hpp's).  The statement, the arguments and the outputs are sph3d_lovasz_softmax's, word for word, `order`
 * included; scope "batch" of the Python surface is this entry on the call reshaped to one block of B N rows.
 *   keys      as sph3d_lovasz_softmax: bits(e) | ~n | fg per valid row, 0 otherwise; runs of `tile` keys are sorted in LDS, then
 *             merged pairwise in ceil(log2(runs)) launches (merge path, 1024 output keys per workgroup).  Valid keys are distinct,
 *             so the sorted order is the statement's order exactly
 *   probs, order, coef   the bits sph3d_lovasz_softmax writes wherever both entries cover the shape (g, U, F: the same integers
 *             and the same fp32 operations)
 *   class_loss  sum_j e_(j) g_j in this tree: the 1024 positions of a tile by the 6-step butterfly over a wave's lanes, then the
 *             16 waves in order onto 0.f; the tiles t = l, l + 64, ... in order onto 0.f in lane l of one wave; the 64 lanes by
 *             the 6-step butterfly.  Longest path: 6 + 15 + (ceil(tiles / 64) - 1) + 6 additions, tiles = ceil(N / tile) tile / 1024
 *   loss, dlogits   as sph3d_lovasz_softmax
 * Classes pass through the sort `slab` at a time, so the workspace holds slab B segments of keys (twice), not C B; the counts
 * G[b,c] are integers, the float reductions run in the fixed order above: the same inputs give the same bits on every run and
 * for every slab.  No float atomics; no workgroup waits for another.
 * tile_log2: 0 (the default, 12: 4096 keys, 32 KB of LDS) or 10..14; slab: 0 (the plan's choice: as many classes as keep the
 * workspace under 128 MB, at least one) or 1..C.  Both exist for tests: forced values reach every merge shape at small N.
 * workspace: sph3d_lovasz_softmax_large_workspace(B, N, C) bytes (for tile_log2 = slab = 0; a forced call asks the plan), 16-byte
 * aligned, dead when the call's last kernel has run.  sph3d_lovasz_softmax_large_plan writes SPH3D_LOVASZ_PLAN_FIELDS values:
 *   tile_log2, tile, runs, npad, passes, mtile, mtiles, slab, slabs, probs_grid, count_grid, sort_lds, merge_lds, grad_grid,
 *   key_bufs, workspace_bytes, off_keys0, off_keys1, off_tilecnt, off_partial, off_count, off_bad, cap
 * (csrc/lovasz_plan.hpp: LovaszPlan says what each is; all 0 for B == 0).
 * N <= 2^20 and C <= 1024: sph3d_lovasz_softmax_large_supported(N, C) -> 1 | 0 on the host.
 * -> SPH3D_OK; SPH3D_EINVAL for B < 0, N <= 0, C <= 0, B N C > 2^40, B C >= 2^31, B >= 2^16; SPH3D_EUNSUPPORTED for N > 2^20 or
 * C > 1024; SPH3D_EINVAL for a tile_log2 or slab outside the above, in this order and before the pointers are looked at; then
 * SPH3D_EINVAL for a null pointer other than inner, dlogits and order, SPH3D_EWORKSPACE for a workspace that is null, too small
 * or not aligned. */
#define SPH3D_LOVASZ_PLAN_FIELDS 23
int sph3d_lovasz_softmax_large_supported(int N, int C);
size_t sph3d_lovasz_softmax_large_workspace(int B, int N, int C);
int sph3d_lovasz_softmax_large_plan(int B, int N, int C, int tile_log2, int slab, long long* out);
int sph3d_lovasz_softmax_large(int B, int N, int C, const float* logits, const long long* label, const float* inner,
                               long long ignore, float* probs, float* coef, float* class_loss, float* loss, float* dlogits,
                               int* order, void* workspace, size_t workspace_bytes, int tile_log2, int slab, sph3d_stream_t stream);

/* softmax cross-entropy with class weights, label smoothing and an ignore label, per block, and its gradient with respect to the
 * logits (csrc/xent.hip; the float64 statement is harness/xent.py: xent_reference).  It is not an op of the reference tree.
 * logits [B,N,C] fp32; label [B,N] int32 (label_bits = 32, as the feeds yield them) or int64 (label_bits = 64); inner [B,N] fp32 or
 * NULL (every row); weight [C] fp32, finite and >= 0, or NULL (all 1); eps = label_smoothing in [0, 1).  Per block b, with
 * p = softmax(x) and lse = log sum exp x of a row:
 *   counted  row n counts iff (inner == NULL or inner[b,n] > 0; NaN > 0 is false) and (has_ignore == 0 or label[b,n] != ignore)
 *   targets  t[n,c] = (1 - eps) w_y [c == y] + (eps / C) w_c,  A_n = sum_c t[n,c]
 *   row      l_n = sum_c t[n,c] (lse_n - x[n,c]), computed as (1 - eps) w_y ((m + logf(se)) - x_y) + (eps / C) sum_c w_c (lse - x_c)
 *            (ascending c; with eps == 0 the first product alone, without the factor)
 *   hist     hist[b,c] = #{counted n: label = c}, int32, exact
 *   D_b      normalize 0 ("count"): (float)(sum_c hist[b,c]);  1 ("weight"): (float)(sum_c (double)hist[b,c] (double)w_c), ascending c
 *   outputs  loss_part[b * S + s], S = sph3d_softmax_xent_parts(N): the shares of S slices of the block's rows in
 *            loss_b = sum_{counted n} l_n / D_b;  dlogits[b,n,:] = (A_n p - t[n,:]) / D_b, computed as
 *            expf(x - m) * ((A * inv) / se) - t * inv with inv = 1 / D_b, on counted rows and exact zeros elsewhere.
 *            D_b == 0: inv = 0, so the loss and the gradient are zeros.  dlogits == NULL: the losses and hist only.
 * A counted row whose label lies outside [0, C) is in no class of hist; it makes its part of loss_part and its own gradient row
 * NaN, and every read stays in range.  With weight == NULL, eps == 0, has_ignore == 0, normalize == 0, int64 labels and a mask,
 * loss_part and dlogits are sph3d_masked_softmax_xent's bit for bit for N <= 16384 (S is then the same; beyond it S keeps growing:
 * ceil(N / 1024), at most 256).  Two launches, fixed-order reductions, integer LDS atomics only: the same inputs give the same
 * bits.  workspace: sph3d_softmax_xent_workspace(B, N, C) bytes (the slices' histograms), 4-byte aligned, the caller's; dead when
 * the call's kernels are done.  C <= 4096 (weights and histogram live in LDS): sph3d_softmax_xent_supported(N, C) -> 1 | 0.
 * -> SPH3D_OK; SPH3D_EINVAL for bad dims (B < 0, N <= 0, C <= 0, B >= 2^16, N > 2^30, B N >= 2^31), label_bits, eps or normalize, or a null
 * pointer other than inner, weight and dlogits; SPH3D_EUNSUPPORTED before the pointers are looked at; SPH3D_EWORKSPACE. */
int sph3d_softmax_xent_parts(int N);
int sph3d_softmax_xent_supported(int N, int C);
size_t sph3d_softmax_xent_workspace(int B, int N, int C);
int sph3d_softmax_xent(int B, int N, int C, const float* logits, const void* label, int label_bits, const float* inner,
                       const float* weight, float label_smoothing, int has_ignore, long long ignore, int normalize,
                       float* loss_part, int* hist, float* dlogits, void* workspace, size_t workspace_bytes, sph3d_stream_t stream);

/* ---- the augmentation stage (csrc/augment.hip; harness/augment.py states it in numpy): the indoor-segmentation recipes published
 * since the reference (chromatic auto-contrast, translation and jitter, colour drop, flips, anisotropic scaling, elastic
 * distortion, Mix3D scene mixing), applied IN PLACE to an assembled batch.  points [B,N,C] fp32 with xyz in channels 0:3, C in
 * {3, 6, 9}; label [B,N] int32; inner [B,N] int32 or NULL.  Every draw is a pure function of (seed, step, b, purpose, counter) of
 * csrc/feed_draws.hpp, purposes 32..38.  Bit k of cloud b is on iff bit k of `enable` is set and the high word of
 * draw(ck_b, 32, k) is below threshold[k] (an integer comparison; threshold in [0, 2^32]); MIX (bit 0) is gated once per pair
 * (2i, 2i+1) from the even cloud's key.  Order on the destination cloud: MIX, FLIPX, FLIPY, ASCALE, ELASTIC (two passes), then
 * AUTOCONTRAST, CTRANSLATE, CJITTER, CDROP on the three channels at rgb_offset.  A cloud whose gates are all off is copied bit
 * for bit.  Integer outputs (label, inner, which slot came from which cloud, the counters) equal the numpy statement bit for bit.
 *   params      by value.  rgb_offset / normal_offset: first channel of the colour / the normal, -1 for none.  inv_g[p] =
 *               (float)(1 / g_p), scale[p] = (float)(mag_p / (729 * 2^20)): the blurred lattice is kept as exact integers.
 *               max_nodes: the largest node box (cells + 5 per axis) a cloud's lattice may take.
 *   workspace   sph3d_augment_workspace(B, N, max_nodes) bytes, 16-byte aligned, the caller's; dead when the call's kernels are done.
 *   status      [3] int64 or NULL, accumulated, never zeroed or read here: elastic passes skipped [0], [1]; pairs mixed [2].
 * Nothing is allocated, nothing is read back, no floating-point atomic is used: the per-cloud statistics are min / max of floats
 * per half cloud (one workgroup each) and integer atomic min / max of cell indices.  At most six launches on `stream`.
 * SPH3D_EINVAL: C, an offset, a threshold, max_nodes (< 216 or > 2^24), the colour range, a colour bit without rgb_offset, the
 * alignment or the workspace size. */
typedef struct sph3d_augment_params {
    unsigned long long threshold[9];
    unsigned int enable;
    int rgb_offset, normal_offset, max_nodes;
    float rgb_lo, rgb_hi;
    float inv_g[2], scale[2];
} sph3d_augment_params;
size_t sph3d_augment_workspace(int B, int N, int max_nodes);
int sph3d_augment_apply(int B, int N, int C, float* points, int* label, int* inner, unsigned long long seed,
                        unsigned long long step, sph3d_augment_params params, void* workspace, size_t workspace_bytes,
                        long long* status, sph3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPH3D_H */
