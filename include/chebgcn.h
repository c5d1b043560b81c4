/*
 * chebgcn.h -- C ABI of libchebgcn.so: the MI355X (gfx950) implementation of the
 * Chebyshev graph-convolution hot path of zhangyu2ustc/GCN_fmri_decoding.
 *
 * The reference has no FFI of its own: the path is a Python class
 * (lib_new/models_gcn.py, class cgcnn) whose methods emit TensorFlow ops.  Each
 * entry point below replaces the TF ops emitted by the cited reference lines;
 * gcn_fmri_decoding_amd/ (Python, ctypes) binds them behind the reference's
 * cgcnn / chebyshev5 / b1relu / b2relu / mpool1 API.  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C types only; every function returns 0 on success or a negative
 *    CHEBGCN_E* code, never throws; chebgcn_last_error() gives the message of
 *    the last failure on the calling thread.
 *  - all activation pointers are DEVICE pointers owned by the caller (PyTorch's
 *    caching allocator in our host code); kernels are enqueued on `stream`
 *    (a hipStream_t; NULL = the default stream) and the call returns without
 *    synchronising.  Pointers marked "host" are host memory, read before return.
 *  - activation layout is "plane": a logical [B, M, F] tensor of the reference
 *    (B windows, M graph vertices, F features) is stored as [B][F][Mp] floats
 *    with the vertex axis fastest and Mp = chebgcn_plane_stride(M) >= M.  The pad
 *    [M, Mp) of every plane is scratch: kernels may write it and never read it
 *    as data.
 *  - a graph handle is immutable after creation and may be used concurrently.
 */
#ifndef CHEBGCN_H
#define CHEBGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHEBGCN_VERSION 1

enum {
    CHEBGCN_OK = 0,
    CHEBGCN_EINVAL = -1,       /* bad argument / shape */
    CHEBGCN_EHIP = -2,         /* a HIP runtime call failed */
    CHEBGCN_ENOMEM = -3,
    CHEBGCN_EUNSUPPORTED = -4  /* valid but not implemented for this size */
};

enum { CHEBGCN_BIAS_NONE = 0, CHEBGCN_BIAS_FILTER = 1 /* b1relu: [F] */, CHEBGCN_BIAS_VERTEX = 2 /* b2relu: [F][Mp] */ };
enum { CHEBGCN_POOL_MAX = 0, CHEBGCN_POOL_AVG = 1 };

typedef struct chebgcn_graph chebgcn_graph;
typedef void* chebgcn_stream;

int chebgcn_version(void);
const char* chebgcn_last_error(void);
/* Names of the kernel templates the calling thread's last launching entry point enqueued, in launch order, joined by
 * " + " (e.g. "contract_bwd_w_kernel<5,true> + reduce_partials_stage1 + reduce_partials_stage2"); "" before the first
 * launch.  The dispatchers below choose instantiations by shape and by the device's CU count: this is how a test (or a
 * profile) names the one a given call reached.  The pointer stays valid until the thread's next call of this function. */
const char* chebgcn_last_dispatch(void);

/* Padded plane length for M vertices (multiple of 32 floats = 128 B). */
int chebgcn_plane_stride(int M);

/* ---- graph: the constant operand of tf.sparse_tensor_dense_matmul ---------------
 * Replaces models_gcn.py:593-596 (tf.SparseTensor + tf.sparse_reorder of the
 * rescaled Laplacian).  Takes L~ = rescale_L(L, lmax=2) (lib_new/graph.py:146-152)
 * as host CSR (row-major, any column order inside a row), builds device-side
 * length-sorted sliced-ELL images of L~ and of L~^T (the adjoint used by the gradient of
 * SparseTensorDenseMatMul).  The order in which the entries of a row are summed is chosen
 * by the library (LDS bank placement), not the caller's: a row sum is an fp32 fmaf chain
 * over its <= ~17 entries in that fixed order, deterministic from run to run.  The host
 * arrays are copied; the caller keeps ownership. */
int chebgcn_graph_create(int M, int64_t nnz, const int32_t* rowptr /*host [M+1]*/,
                         const int32_t* colidx /*host [nnz]*/, const float* vals /*host [nnz]*/,
                         chebgcn_graph** out);
/* The same, with the number of planes (window x feature columns) a recurrence workgroup carries
 * on chip chosen by the caller: 0 = automatic (what chebgcn_graph_create does: 4 wherever 16 bytes
 * per active vertex fit the 160 KB of LDS, i.e. up to ~10200 active vertices, else 2), 2, or 4
 * (CHEBGCN_EUNSUPPORTED where 4 do not fit).  The
 * choice affects speed and the order of the terms inside a row sum (results agree to fp32
 * round-off).  With 0, a graph that fits four planes keeps a two-plane image as well and a launch
 * of fewer than four plane groups per CU (ceil(B*Fin/4) < 4 * CUs) runs on it: the same window can
 * then differ in its last fp32 bits between batch sizes (training batch, evaluation batch, a
 * data-parallel shard) and between GPUs with different CU counts; planes = 2 or 4 pins one image. */
int chebgcn_graph_create_planes(int M, int64_t nnz, const int32_t* rowptr, const int32_t* colidx,
                                const float* vals, int planes, chebgcn_graph** out);
void chebgcn_graph_destroy(chebgcn_graph* g);
/* what: 0 = M, 1 = nnz, 2 = plane stride Mp, 3 = 1 if the on-chip (LDS) recurrence
 * kernel is used for this graph, 4 = padded ELL slots of L~, 5 = max row length,
 * 6 = planes per workgroup (0, 2, 4), 7 = rows held in the LDS image, 8 = LDS bytes of the
 * image, 9 / 10 / 11 = modelled LDS cycles of one gather pass in the caller's entry order /
 * after the library's bank-aware placement / without any conflict, 12 = 1 if the handle carries
 * the ORDERED operator image: the rows of the caller's matrix are sorted by descending length
 * (isolated vertices last) and the graph was created with planes = 0 -- recurrence launches then
 * run the kernel that moves planes between HBM and registers directly (csrc/recurrence_ord_kernel.h;
 * served: planes of more than 1024 vertices, up to 20476 active ones -- 256 threads per workgroup up to 2048 active vertices
 * (forward recurrences only: the Clenshaw adjoint of such a graph runs the kernel of the caller's order), 512 beyond --, any
 * number of isolated / padding vertices behind them);
 * 13 / 14 / 15 = items 9 / 10 / 11 for that image, 16 = its planes per workgroup (4 up to 10238
 * active vertices, 2 beyond; 0 = no ordered image). */
int chebgcn_graph_query(const chebgcn_graph* g, int what, int64_t* value);

/* ---- Chebyshev recurrence, forward: models_gcn.py:598-610 -----------------------
 * T_0 = x, T_1 = L~ T_0, T_k = 2 L~ T_{k-1} - T_{k-2}.
 * x: [B][Fin][Mp]; stack: [K][B][Fin][Mp].  Slab 0 receives a copy of x unless
 * x == stack (the producer already wrote T_0 in place). */
int chebgcn_recurrence_fwd(const chebgcn_graph* g, const float* x, float* stack,
                           int B, int Fin, int K, chebgcn_stream stream);

/* ---- the same recurrence on the TRANSPOSED operator: T_k(L~^T) x ------------------------------
 * (TF autodiff of models_gcn.py:598-617, associated the other way round.)  The gradient of a layer wrt its input is
 *   dx[b][fin] = sum_{k,fo} W[fin*K+k][fo] * ( T_k(L~^T) dy[b][fo] )
 * -- the forward recurrence on the Fout planes of dy, then chebgcn_contract_fwd(_bf16) of that stack with the re-indexed
 * weights W'[fo*K+k][fin] = W[fin*K+k][fo].  For Fout <= Fin this moves no more bytes than chebgcn_contract_bwd_x +
 * chebgcn_recurrence_bwd (which compute the same sum in Clenshaw form) and runs on the two faster kernels.  Same layouts and
 * in-place rule as chebgcn_recurrence_fwd. */
int chebgcn_recurrence_fwd_t(const chebgcn_graph* g, const float* x, float* stack,
                             int B, int Fin, int K, chebgcn_stream stream);
/* the re-indexed weights of that contraction: Wt[(fo*K + k)*Fin + fin] = W[(fin*K + k)*Fout + fo]  ([Fout*K][Fin] from
 * [Fin*K][Fout], both row-major; one small launch -- the weights change every step) */
int chebgcn_reindex_weights(const float* W, float* Wt, int Fin, int K, int Fout, chebgcn_stream stream);
/* The same for n <= 16 layers in one launch (host arrays of device pointers and shapes): the weights are constant within a
 * training step, cgcnn re-indexes every layer that forms its input gradient this way once, in front of the backward pass. */
int chebgcn_reindex_weights_batch(int n, const float* const* W, float* const* Wt, const int* Fin, const int* K,
                                  const int* Fout, chebgcn_stream stream);
/* The contraction of that stack with the ReluGrad of the layer BELOW in its epilogue (TF autodiff chains the two:
 * models_gcn.py:616 MatMul gradient -> :625/:629 ReluGrad of the previous layer): out[b][fo][m] = gate bit ? sum : 0, `gate` a
 * ReLU mask as chebgcn_contract_fwd leaves it, [B][Fout][Mp/4].  With stack = T_k(L~^T) dy of layer l and W = W' of layer l,
 * `out` IS the gated gradient wrt the output of layer l-1 -- written straight into slab 0 of the stack its own
 * chebgcn_recurrence_fwd_t fills, so the separate ReluGrad pass of layer l-1 (chebgcn_brelu_pool_bwd writing dy) shrinks to the
 * bias reduction.  No bias, no ReLU, no pooling; Fout <= 32 on a big launch (chebgcn_contract_fwd_gated_supported),
 * CHEBGCN_EUNSUPPORTED otherwise.  Same products in the same order as chebgcn_contract_fwd: bit-identical to
 * chebgcn_contract_fwd followed by the gating pass. */
int chebgcn_contract_fwd_gated_supported(int B, int M, int Fin, int K, int Fout);
int chebgcn_contract_fwd_gated(const float* stack, const float* W, const uint8_t* gate, float* out, int B, int M,
                               int Fin, int K, int Fout, chebgcn_stream stream);

/* ---- Chebyshev recurrence, adjoint: gradient of the above wrt x -----------------
 * (TF autodiff of models_gcn.py:598-610, reached from :298-303.)
 * c_{K-1} = G_{K-1}; c_j = G_j + 2 L~^T c_{j+1} - c_{j+2}; dx = G_0 + L~^T c_1 - c_2.
 * gstack: [K][B][Fin][Mp] (read only); dx: [B][Fin][Mp]. */
int chebgcn_recurrence_bwd(const chebgcn_graph* g, const float* gstack, float* dx,
                           int B, int Fin, int K, chebgcn_stream stream);

/* ---- dense contraction + bias + ReLU + pooling, forward -------------------------
 * Replaces models_gcn.py:611-617 (transpose/reshape + tf.matmul with W[Fin*K, Fout],
 * row index fin*K + k), :619-629 (b1relu / b2relu) and :631-648 (mpool1 / apool1).
 * stack: [K][B][Fin][Mp(M)];  W: [Fin*K][Fout] row-major;  bias: [Fout] or
 * [Fout][Mp(M)] or NULL;  out: [B][Fout][Mp(M/pool)];  argmax (may be NULL, only
 * written for max pooling with pool > 1): [B][Fout][Mp(M/pool)] bytes, position of
 * the first maximum inside each window.  relu != 0 applies max(.,0) before pooling.
 * pool must be a power of two <= 128 and divide M.
 * pool == 1 with relu != 0: a non-NULL argmax receives the ReLU MASK, [B][Fout][Mp(M)/4] bytes,
 * bit r of byte i = (out[4i+r] > 0) -- all that the gradient entries *_relu below need of the
 * forward result. */
int chebgcn_contract_fwd(const float* stack, const float* W, const float* bias, int bias_kind,
                         float* out, uint8_t* argmax, int B, int M, int Fin, int K, int Fout,
                         int pool, int pool_kind, int relu, chebgcn_stream stream);

/* ---- the same contraction over WINDOWS of one longer stack (decoding a scan window by window: cgcnn.decode_series) ------
 * The first layer's input folds time into the channels (x[b][m][c] = s[starts[b] + c][m]) and the recurrence acts on every
 * channel plane on its own, so overlapping windows share their Chebyshev planes:
 *   stack: [K][T][Mp(M)], what chebgcn_recurrence_fwd(g, s, stack, 1, T, K) leaves for the T time points of a scan;
 *   starts: int32 [B] on the device; window b contracts the planes of the time points starts[b] .. starts[b] + C - 1:
 *     y[b][o][m] = act( sum_{c<C, k<K} W[c*K + k][o] * stack[k][starts[b] + c][m] + bias ) -> pool over m
 *   W, bias, out, argmax, pool, pool_kind, relu: exactly as chebgcn_contract_fwd with Fin = C.
 * Every start must satisfy 0 <= start and start + C <= T: the CALLER checks the table before it uploads it (the library
 * cannot read it without a synchronisation); a start outside that range is moved into it by the kernel, which therefore
 * never reads outside the stack.  Overlapping, repeated and unsorted starts are fine.  Forward only.
 * fp32 matrix instructions, Fout <= 32 (chebgcn_contract_fwd_windows_supported; CHEBGCN_EUNSUPPORTED otherwise).  Served: the
 * three forward arms chebgcn_contract_fwd has for Fout <= 32, chosen by the same rules, reported by chebgcn_last_dispatch() as
 *   contract_fwd_windows_splitk_kernel       small launches (ceil(M/512) * B < 2 * CUs), any pool
 *   contract_fwd_windows_ring_kernel         big launches, pool == 1, C*K up to 352 rows (and Fout >= 4 with a per-filter bias)
 *   contract_fwd_windows_ring_kernel<pool>   the same with pooling
 *   contract_fwd_windows_kernel<1>           big launches beyond the ring kernel's shapes
 * Same products in the same order as chebgcn_contract_fwd: BIT-IDENTICAL to it on the gathered [K][B][C][Mp] stack; with
 * starts = {0, C, 2C, ...} and T = B*C the two read the very same memory. */
int chebgcn_contract_fwd_windows_supported(int B, int M, int C, int K, int Fout, int pool);
int chebgcn_contract_fwd_windows(const float* stack, int64_t T, const int32_t* starts, const float* W, const float* bias,
                                 int bias_kind, float* out, uint8_t* argmax, int B, int M, int C, int K, int Fout, int pool,
                                 int pool_kind, int relu, chebgcn_stream stream);

/* ---- the same contraction on the bf16 matrix cores (wide layers: block_dura = 60, Fout = 256,
 * where the fp32-input MFMA is compute bound).  Same operands, epilogue and results layout as
 * chebgcn_contract_fwd; fp32 in HBM, converted in registers, fp32 accumulate.
 * passes = 1: operands rounded to bf16;  passes = 3: operands split into two bf16 each and
 * hi*hi + hi*lo + lo*hi accumulated (fp32-grade results, three times the matrix work).
 * workspace: device scratch of at least chebgcn_contract_fwd_bf16_workspace(Fin, K, Fout) bytes
 * (the packed bf16 image of W, rebuilt on every call). */
size_t chebgcn_contract_fwd_bf16_workspace(int Fin, int K, int Fout);
int chebgcn_contract_fwd_bf16(const float* stack, const float* W, const float* bias, int bias_kind,
                              float* out, uint8_t* argmax, int B, int M, int Fin, int K, int Fout,
                              int pool, int pool_kind, int relu, int passes, void* workspace,
                              size_t workspace_bytes, chebgcn_stream stream);

/* ---- the two gradients of the contraction on the bf16 matrix cores (wide layers; replace the
 * MatMul gradient TensorFlow derives for models_gcn.py:616 when the layer computes in bf16).
 * Same operands, layouts and `passes` as above; fp32 in HBM, fp32 accumulate, deterministic.
 *   bwd_x: gstack[k][b][fin][m] = sum_o  W[fin*K+k][o] * dy[b][o][m]     (overwrites gstack)
 *   bwd_w: dW[fin*K+k][o]       = sum_{b,m} stack[k][b][fin][m] * dy[b][o][m]   (overwrites dW)
 * Workspaces: device scratch of at least the size the *_workspace function reports. */
size_t chebgcn_contract_bwd_x_bf16_workspace(int Fin, int K, int Fout);
int chebgcn_contract_bwd_x_bf16(const float* dy, const float* W, float* gstack, int B, int M, int Fin,
                                int K, int Fout, int passes, void* workspace, size_t workspace_bytes,
                                chebgcn_stream stream);
size_t chebgcn_contract_bwd_w_bf16_workspace(int B, int M, int Fin, int K, int Fout);
int chebgcn_contract_bwd_w_bf16(const float* stack, const float* dy, float* dW, void* workspace,
                                size_t workspace_bytes, int B, int M, int Fin, int K, int Fout,
                                int passes, chebgcn_stream stream);

/* ---- the same two gradients with dy handed over as bf16 (one-pass arithmetic, wide layers).
 * The one-pass kernels round dy to bf16 before it meets the matrix cores; when the ReluGrad pass that produces dy
 * (models_gcn.py:619-629 under TF autodiff) writes it as bf16 in the first place, the largest operand of both gradients is half
 * the bytes and the results are BIT-IDENTICAL to chebgcn_contract_bwd_*_bf16(passes = 1) on the fp32 dy.
 *   chebgcn_relu_grad_bf16: dy16[b][o][m] = bf16( relu_mask bit ? dout[b][o][m] : 0 ), planes [B][F][Mp(M)] of 2-byte
 *       elements, and the bias gradient (fp32, fixed-order sums) in the same pass; relu_mask as chebgcn_contract_fwd(_bf16)
 *       wrote it for a pool == 1 ReLU layer; workspace as for chebgcn_brelu_pool_bwd.
 *   chebgcn_bf16_dy16_supported: 1 where both gradients below take this operand (layers wide enough for the one-pass weight
 *       gradient: Fin*K > 160 and Fout > 64), else 0 -- callers then keep the fp32 dy.
 *   workspaces: chebgcn_contract_bwd_w_bf16_workspace / chebgcn_contract_bwd_x_bf16_workspace. */
int chebgcn_relu_grad_bf16(const float* dout, const uint8_t* relu_mask, uint16_t* dy16, float* dbias, int bias_kind,
                           int B, int M, int F, void* workspace, size_t workspace_bytes, chebgcn_stream stream);
int chebgcn_bf16_dy16_supported(int B, int M, int Fin, int K, int Fout);
int chebgcn_contract_bwd_w_bf16_dy16(const float* stack, const uint16_t* dy16, float* dW, void* workspace,
                                     size_t workspace_bytes, int B, int M, int Fin, int K, int Fout,
                                     chebgcn_stream stream);
int chebgcn_contract_bwd_x_bf16_dy16(const uint16_t* dy16, const float* W, float* gstack, int B, int M, int Fin,
                                     int K, int Fout, void* workspace, size_t workspace_bytes, chebgcn_stream stream);

/* ---- bias + ReLU + pooling on their own (b1relu / b2relu / mpool1 / apool1 called
 * separately, models_gcn.py:619-648); same conventions as the epilogue of contract_fwd.
 * x: [B][F][Mp(M)] -> out: [B][F][Mp(M/pool)]. */
int chebgcn_brelu_pool_fwd(const float* x, const float* bias, int bias_kind, float* out,
                           uint8_t* argmax, int B, int M, int F, int pool, int pool_kind,
                           int relu, chebgcn_stream stream);

/* ---- backward of pooling + ReLU + bias (MaxPoolGrad, ReluGrad, bias reductions) ---
 * dout, out: [B][F][Mp(M/pool)] (out = forward result); argmax as written by the
 * forward; dy: [B][F][Mp(M)] receives d(loss)/d(pre-bias activation); dbias: [F] or
 * [F][Mp(M)] (overwritten) or NULL.  pool == 1 with relu: a non-NULL argmax is the ReLU mask of
 * contract_fwd and replaces `out` (which may then be NULL).  dy == NULL: only dbias is computed; with pool == 1 and relu == 0
 * as well that is the plain sum of dout over the windows (per filter: and vertices) -- the bias gradient of a layer whose
 * gated dy the layer above stored (chebgcn_contract_fwd_gated).
 * workspace: device scratch of at least chebgcn_brelu_pool_bwd_workspace() bytes.  bias_kind CHEBGCN_BIAS_FILTER needs
 * it: the per-filter sum of b1relu (models_gcn.py:619-623) is a two-stage reduction in a fixed order (per-workgroup
 * partials, then one wave per filter), so every gradient this library returns is bit-reproducible from run to run.  A
 * pooled layer (pool > 1) WITH the workspace runs the 16-byte-store kernel of chebgcn_pool_scatter_bwd (its bias sums
 * are per-batch-part partials added in part order); without it (NULL allowed for the other bias kinds) a scalar kernel. */
size_t chebgcn_brelu_pool_bwd_workspace(int B, int M, int F, int pool, int bias_kind);
int chebgcn_brelu_pool_bwd(const float* dout, const float* out, const uint8_t* argmax,
                           float* dy, float* dbias, int bias_kind, int B, int M, int F,
                           int pool, int pool_kind, int relu, void* workspace, size_t workspace_bytes,
                           chebgcn_stream stream);

/* ---- pooling between two vertex orders (mpool1 / apool1, models_gcn.py:631-648, under a relabelling) ----
 * The reference pools `pool` CONSECUTIVE vertices of the tree order coarsening.compute_perm builds (coarsening.py:168-215).
 * A caller that keeps the vertices of a level in another order -- cgcnn relabels each level by descending row length so that
 * the ordered recurrence kernels serve it (HCP_task_fmri_gcn_test8.py:1632-1635: the six-level pooling network) -- pools
 * through index maps instead of through adjacency in memory:
 *   chebgcn_pool_gather_fwd: y [B][F][Mp(M)] (bias and ReLU already applied: chebgcn_contract_fwd with pool = 1) ->
 *       out[b][f][j] = max_i / mean_i  y[b][f][ pmap[j*pool + i] ],  j < M/pool, [B][F][Mp(M/pool)] (padding zeroed).
 *       pmap: int32 [M] on the device, positions in the source order, the members of a cluster listed in the reference's
 *       order (ties resolve alike); NULL = the identity (the tree order itself).  sel [B][F][Mp(M/pool)] (optional, for the
 *       gradient): max -- the winning member, 0xFF where `relu` says y was rectified and the maximum is not positive;
 *       average -- bit i set where member i was positive (pool <= 8).
 *   chebgcn_pool_scatter_bwd: dy[b][f][v] = gradient of source vertex v (MaxPoolGrad / AvgPoolGrad + ReluGrad) from
 *       dout [B][F][Mp(M/pool)] and sel; smap: int32 [M], smap[v] = j*pool + i (v is member i of pooled vertex j), NULL =
 *       the identity; sel may be NULL for the average without ReLU (every member takes its share, at any pool), and the
 *       average with ReLU is refused beyond pool 8 (its mask holds 8 members); dbias as chebgcn_brelu_pool_bwd (fixed-order
 *       sums: per-batch-part partials in `workspace`, at least chebgcn_pool_scatter_bwd_workspace() bytes, added in part order).  16-byte stores of dy; the pooled plane is staged
 *       in LDS, so planes of more than 10240 pooled vertices are refused (CHEBGCN_EINVAL). */
int chebgcn_pool_gather_fwd(const float* y, const int32_t* pmap, float* out, uint8_t* sel, int B, int M, int F,
                            int pool, int pool_kind, int relu, chebgcn_stream stream);
size_t chebgcn_pool_scatter_bwd_workspace(int B, int M, int F, int pool, int bias_kind);
int chebgcn_pool_scatter_bwd(const float* dout, const uint8_t* sel, const int32_t* smap, float* dy, float* dbias,
                             int bias_kind, int B, int M, int F, int pool, int pool_kind, int relu, void* workspace,
                             size_t workspace_bytes, chebgcn_stream stream);

/* ---- gradients of the contraction (MatMul grads) ---------------------------------
 * dW[fin*K+k][o] = sum_{b,m} stack[k][b][fin][m] * dy[b][o][m]      (overwritten)
 * gstack[k][b][fin][m] = sum_o dy[b][o][m] * W[fin*K+k][o]
 * workspace: device scratch of at least chebgcn_contract_bwd_w_workspace() bytes. */
size_t chebgcn_contract_bwd_w_workspace(int B, int M, int Fin, int K, int Fout);
int chebgcn_contract_bwd_w(const float* stack, const float* dy, float* dW, void* workspace,
                           size_t workspace_bytes, int B, int M, int Fin, int K, int Fout,
                           chebgcn_stream stream);
/* The same two gradients with the ReluGrad of the reference's autodiff folded in (pool == 1
 * layers): dout = d(loss)/d(layer output) [B][Fout][Mp], relu_mask as written by contract_fwd;
 * dy = dout where the mask bit is set, else 0, is formed in registers and never stored.  The bias
 * gradient of such a layer: chebgcn_brelu_pool_bwd(dout, NULL, relu_mask, dy = NULL, dbias, ...). */
int chebgcn_contract_bwd_w_relu(const float* stack, const float* dout, const uint8_t* relu_mask,
                                float* dW, void* workspace, size_t workspace_bytes, int B, int M,
                                int Fin, int K, int Fout, chebgcn_stream stream);
/* chebgcn_contract_bwd_w_relu with the per-vertex bias gradient of the layer (b2relu, models_gcn.py:625-629: dbias[o][m] = sum over
 * the windows of the gated dout, [Fout][Mp]) in its second launch -- the one that adds the per-workgroup partials of dW: an
 * atlas-sized layer's backward is a chain of ~5 us launches, and chebgcn_brelu_pool_bwd(dout, NULL, relu_mask, NULL, dbias, ...) was
 * one of them.  Same sums in the same order as the two calls it replaces.  Served where chebgcn_contract_bwd_w_relu_bias_merged()
 * returns 1 (few partials -- a small launch -- and the bias reduction's small-graph shape); CHEBGCN_EUNSUPPORTED otherwise. */
int chebgcn_contract_bwd_w_relu_bias_merged(int B, int M, int Fin, int K, int Fout);
int chebgcn_contract_bwd_w_relu_bias(const float* stack, const float* dout, const uint8_t* relu_mask,
                                     float* dW, float* dbias, void* workspace, size_t workspace_bytes,
                                     int B, int M, int Fin, int K, int Fout, chebgcn_stream stream);
int chebgcn_contract_bwd_x_relu(const float* dout, const uint8_t* relu_mask, const float* W,
                                float* gstack, int B, int M, int Fin, int K, int Fout,
                                chebgcn_stream stream);
int chebgcn_contract_bwd_x(const float* dy, const float* W, float* gstack, int B, int M,
                           int Fin, int K, int Fout, chebgcn_stream stream);

/* ---- last conv layer + tf.reduce_mean(x, -1) (models_gcn.py:673) in one pass ----------------
 * The mean over the filters of the layer's (bias + ReLU) result is all the head reads (models_gcn.py:671-674), so the
 * last layer need not store its [B][Fout][Mp] output at all:
 *   chebgcn_contract_fwd_mean: mean_out[b][m] = (1/Fout) sum_o relu(y[b][o][m] + bias), [B][Mp]; relu_mask as
 *     chebgcn_contract_fwd writes it (may be NULL for inference).  pool = 1, ReLU.  Served where
 *     chebgcn_contract_fwd_mean_supported() returns 1 (4 <= Fout <= 32, a big launch, Fin*K*136 bytes <= 48 KB);
 *     CHEBGCN_EUNSUPPORTED otherwise (run chebgcn_contract_fwd + chebgcn_feature_mean_fwd).
 *   backward: d(loss)/d(y[b][o][m]) = gmean[b][m] for EVERY filter o, gmean = d(loss)/d(mean) / Fout, [B][Mp] (zero in the
 *     padding): the three gradients of a ReLU-folded layer read that one plane per window instead of a [B][Fout][Mp]
 *     tensor -- the _mean forms of chebgcn_contract_bwd_w_relu / _bwd_x_relu and of the bias reduction
 *     chebgcn_brelu_pool_bwd(dout, NULL, relu_mask, NULL, dbias, ...). */
int chebgcn_contract_fwd_mean_supported(int B, int M, int Fin, int K, int Fout);
int chebgcn_contract_fwd_mean(const float* stack, const float* W, const float* bias, int bias_kind,
                              float* mean_out, uint8_t* relu_mask, int B, int M, int Fin, int K, int Fout,
                              chebgcn_stream stream);
int chebgcn_contract_bwd_w_relu_mean(const float* stack, const float* gmean, const uint8_t* relu_mask,
                                     float* dW, void* workspace, size_t workspace_bytes, int B, int M,
                                     int Fin, int K, int Fout, chebgcn_stream stream);
int chebgcn_contract_bwd_x_relu_mean(const float* gmean, const uint8_t* relu_mask, const float* W,
                                     float* gstack, int B, int M, int Fin, int K, int Fout,
                                     chebgcn_stream stream);
int chebgcn_bias_grad_relu_mean(const float* gmean, const uint8_t* relu_mask, float* dbias, int bias_kind,
                                int B, int M, int F, void* workspace, size_t workspace_bytes,
                                chebgcn_stream stream);
/* The same pass also writing the gated gradient dy[b][o][m] = relu_mask bit ? gmean[b][m] : 0, [B][F][Mp] -- the input of
 * chebgcn_recurrence_fwd_t when the layer's gradient wrt its input is formed by the forward recurrence on dy. */
int chebgcn_relu_grad_mean(const float* gmean, const uint8_t* relu_mask, float* dy, float* dbias, int bias_kind,
                           int B, int M, int F, void* workspace, size_t workspace_bytes,
                           chebgcn_stream stream);

/* ---- atlas-sized graphs: one Chebyshev layer per launch, on chip ---------------------------------
 * models_gcn.py:587-629 (chebyshev5 + b1relu / b2relu, no pooling) for graphs of at most 384 vertices (the
 * reference's own atlases: 246..360 regions, configure_fmri.py:11) and Fin, Fout <= 32: a workgroup carries a whole
 * window through the recurrence in LDS / registers and multiplies every T_k with W_k on the matrix cores while it is
 * still on chip -- the stack is written only if `stack` is non-NULL (training: chebgcn_contract_bwd_w reads it), never
 * read; slab 0 may be x itself.  Same operands, layouts, results (fp32 round-off) and ReLU mask as
 * chebgcn_recurrence_fwd + chebgcn_contract_fwd(pool = 1).  chebgcn_fused_layer_supported() says whether a shape is
 * served (else CHEBGCN_EUNSUPPORTED).
 *   chebgcn_fused_layer_bwd_x: d(loss)/dx of the same layer from d(loss)/d(output) (gated by relu_mask unless NULL):
 *   G_j = dy W_j^T on the matrix cores feeding the adjoint recurrence directly -- replaces chebgcn_contract_bwd_x[_relu]
 *   + chebgcn_recurrence_bwd, no gradient stack in memory. */
int chebgcn_fused_layer_supported(const chebgcn_graph* g, int B, int Fin, int K, int Fout);
/* Device scratch the forward needs (0 for large batches): with fewer than ~3/4 of a window per CU a window is split between
 * two workgroups (half of the input planes each) whose partial sums a second small launch adds in a fixed order. */
size_t chebgcn_fused_layer_workspace(const chebgcn_graph* g, int B, int Fin, int K, int Fout);
int chebgcn_fused_layer_fwd(const chebgcn_graph* g, const float* x, const float* W, const float* bias, int bias_kind,
                            float* stack, float* out, uint8_t* relu_mask, void* workspace, size_t workspace_bytes,
                            int B, int Fin, int K, int Fout, int relu, chebgcn_stream stream);
int chebgcn_fused_layer_bwd_x(const chebgcn_graph* g, const float* dout, const uint8_t* relu_mask, const float* W,
                              float* dx, int B, int Fin, int K, int Fout, chebgcn_stream stream);

/* ---- layout / staging -----------------------------------------------------------
 * perm_data: coarsening.perm_data_3d (lib_new/coarsening.py:244-265) fused with the
 * fp32 cast and batch gather of fit() (models_gcn.py:138-146):
 *   out[s][f][i] = perm[i] < N ? x[sample[s]][perm[i]][f] : 0,   i < M
 * x: [S_total][N][F] row layout (device); perm: int32 [M] (device); sample: int32 [S]
 * (device) or NULL for the identity; out: [S][F][Mp(M)], zero in the pad [M, Mp).
 * perm[i] outside [0, N) gives 0: the coarsening's fake vertices (perm[i] >= N) and negative entries alike; no entry of
 * perm becomes an address unchecked.  sample[s] must lie in [0, S_total): that stays the caller's duty (the entry is not
 * given S_total).  perm NULL: the identity, which needs M == N.
 * to_plane / from_plane convert between the reference's [B][M][F] and plane layout. */
int chebgcn_perm_data(const float* x, const int32_t* perm, const int32_t* sample, float* out,
                      int S, int N, int M, int F, chebgcn_stream stream);
int chebgcn_to_plane(const float* x_bmf, float* out_plane, int B, int M, int F, chebgcn_stream stream);
int chebgcn_from_plane(const float* x_plane, float* out_bmf, int B, int M, int F, chebgcn_stream stream);

/* ---- head: tf.reduce_mean(x, -1) (models_gcn.py:673) and its gradient -----------
 * x: [B][F][Mp(M)] -> y: [B][M] (dense);  dy: [B][M] -> dx: [B][F][Mp(M)]. */
int chebgcn_feature_mean_fwd(const float* x, float* y, int B, int M, int F, chebgcn_stream stream);
int chebgcn_feature_mean_bwd(const float* dy, float* dx, int B, int M, int F, chebgcn_stream stream);

/* ---- head: fully connected layer (models_gcn.py:650-656) -------------------------
 *   y[b][o] = act( sum_i x[b][i] * W[i][o] + bias[o] ),  act = ReLU if relu else identity
 * x: [B] rows of I floats, row stride ldx floats (a [B, M] view of a [B, Mp] buffer is fine; ldx % 4 == 0, x 16-byte
 * aligned, else CHEBGCN_EUNSUPPORTED); W: [I][O] dense; bias: [O] or NULL; y: [B][O] dense.  32 x 32 tiles of y, eight waves
 * split the reduction; long reductions are also split across workgroups (partials in `workspace`,
 * chebgcn_fc_fwd_workspace bytes, 0 for short ones) and added in a fixed order by a second launch.
 * chebgcn_fc_fwd_supported: B*O <= 2^20, I <= 2^20. */
int chebgcn_fc_fwd_supported(int B, int I, int O);
size_t chebgcn_fc_fwd_workspace(int B, int I, int O);
int chebgcn_fc_fwd(const float* x, int64_t ldx, const float* W, const float* bias, float* y, void* workspace,
                   size_t workspace_bytes, int B, int I, int O, int relu, chebgcn_stream stream);
/* The layer's three gradients (TF autodiff of :650-656): with gm = g where y > 0, else 0 (ReluGrad; gm = g if y is NULL)
 *   dW[i][o] = sum_b x[b][i] gm[b][o],   db[o] = sum_b gm[b][o],   dx[b][i] = sum_o gm[b][o] W[i][o]
 * g, y: [B][O] dense; dW: [I][O]; db: [O] or NULL; dx: [B] rows of stride lddx, or NULL (first layer of a model whose input
 * needs no gradient); dW NULL skips dW and db.  Same range as chebgcn_fc_fwd; every sum in a fixed order. */
int chebgcn_fc_bwd(const float* x, int64_t ldx, const float* W, const float* g, const float* y, float* dW, float* db,
                   float* dx, int64_t lddx, int B, int I, int O, chebgcn_stream stream);

/* The flatten of finetuning_cgcnn's head, tf.reshape(conv, [N, M*F]) (models_gcn.py:805-806), and its adjoint:
 *   rows[b][m*F + f] = planes[b][f][v'],  order[v'] = m  (order: int32 [M], the level's internal vertex order -- internal
 *   position -> reference vertex, a permutation; NULL: the identity).
 * planes: [B][F][Mp(M)]; rows: [B] rows of stride ldr >= M*F floats (the columns [M*F, ldr) are not touched).
 * chebgcn_rows_to_planes writes every position of the planes, zero in the pad. */
int chebgcn_planes_to_rows(const float* planes, float* rows, const int32_t* order, int B, int M, int F, int64_t ldr,
                           chebgcn_stream stream);
int chebgcn_rows_to_planes(const float* rows, float* planes, const int32_t* order, int B, int M, int F, int64_t ldr,
                           chebgcn_stream stream);

/* The two scalars a captured training step reads from device memory -- Adam's step size lr_t of this step (models_gcn.py:296:
 * tf.train.AdamOptimizer's lr * sqrt(1 - b2^t) / (1 - b1^t)) and the read factor of the loss average (models_gcn.py:269-275) --,
 * written in one launch in front of the graph's replay: dst[0] = v0, dst[1] = v1. */
int chebgcn_set_scalars(float* dst, float v0, float v1, chebgcn_stream stream);

/* Adam as above (lr_t by value, or read from *lr_t_dev when that is not NULL) which also leaves the sum of squares of the
 * PRE-update variables -- the L2 term of the loss, models_gcn.py:262-266 -- as chebgcn_adam_partials(n) per-workgroup partial
 * sums in sq_partials; and the rest of the loss bookkeeping of a step in one launch:
 *   loss = *cross_entropy + half_reg * sum(sq_partials[0..nparts));   *ema += (1 - decay) * (loss - *ema)   (the
 *   tf.train.ExponentialMovingAverage(0.9) of :269-275);   *loss_average_out = *ema * corr   (corr read from *corr_dev when set:
 *   the zero-debiasing factor 1 / (1 - decay^t));   *loss_out = loss when not NULL.  Fixed-order sums. */
int chebgcn_adam_partials(int64_t n);
int chebgcn_adam_step_sq(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, const float* lr_t_dev,
                         float beta1, float beta2, float eps, float grad_scale, float l2, float* sq_partials,
                         chebgcn_stream stream);
/* ... over ALL variables of a model in one launch: elements [0, n_reg) as chebgcn_adam_step_sq (L2 term l2 * p in the gradient,
 * counted in the sum of squares), elements [n_reg, n) -- the biases, which models_gcn.py:262-266 does not regularise -- plain Adam. */
int chebgcn_adam_step_sq_all(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_reg, float lr_t,
                             const float* lr_t_dev, float beta1, float beta2, float eps, float grad_scale, float l2,
                             float* sq_partials, chebgcn_stream stream);
/* Nadam over one range of a model's variables in one launch: tf.contrib.opt.NadamOptimizer (finetuning_cgcnn, models_gcn.py:
 * 895-933), i.e. TensorFlow's ApplyAdam with use_nesterov:  m += (1-b1)(g'-m);  v += (1-b2)(g'^2-v);
 * p -= (g'(1-b1) + b1 m) lr_t / (sqrt(v)+eps).  Elements [0, n_reg) take the L2 term (g' = grad_scale g + l2 p) and leave the
 * chebgcn_adam_partials(n) partial sums of squares of the PRE-update p in sq_partials (for chebgcn_loss_bookkeeping),
 * elements [n_reg, n) plain Nadam; lr_t by value, or read from *lr_t_dev when that is not NULL.  Fixed-order sums. */
int chebgcn_nadam_step_sq_all(float* p, const float* g, float* m, float* v, int64_t n, int64_t n_reg, float lr_t,
                              const float* lr_t_dev, float beta1, float beta2, float eps, float grad_scale, float l2,
                              float* sq_partials, chebgcn_stream stream);
int chebgcn_loss_bookkeeping(const float* cross_entropy, const float* sq_partials, int nparts, float half_reg, float* ema,
                             float decay, float corr, const float* corr_dev, float* loss_out, float* loss_average_out,
                             chebgcn_stream stream);

/* ---- loss: tf.nn.sparse_softmax_cross_entropy_with_logits + tf.reduce_mean (models_gcn.py:257-259) and its gradient wrt
 * the logits, one launch:  *loss = mean_b( logsumexp(z_b) - z_b[y_b] ),  dlogits[b][c] = (softmax(z_b)[c] - [c == y_b]) / B.
 * logits, dlogits: [B][C] dense; labels: [B] int32 (labels_int64 = 0) or int64 (1), values in [0, C); loss: one float.
 * A label outside [0, C) makes *loss and that row of dlogits NaN (what TensorFlow's GPU kernel returns for it; nothing is
 * read or written outside the row).  Deterministic (fixed-order sums). */
int chebgcn_softmax_xent(const float* logits, const void* labels, int labels_int64, float* loss, float* dlogits, int B,
                         int C, chebgcn_stream stream);

/* ---- optimizer: tf.train.AdamOptimizer step (models_gcn.py:296, TF form) ---------
 * g' = grad_scale * g + l2 * p (per-segment l2 handled by the caller passing
 * segments);  m += (1-b1)(g'-m);  v += (1-b2)(g'^2-v);  p -= lr_t * m / (sqrt(v)+eps)
 * with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller. */
int chebgcn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t,
                      float beta1, float beta2, float eps, float grad_scale, float l2,
                      chebgcn_stream stream);
/* The same step with lr_t read from DEVICE memory when the kernel runs: the form a captured HIP graph of
 * the training step replays (the host writes this step's lr_t into *lr_t_dev ahead of the launch). */
int chebgcn_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_t_dev,
                          float beta1, float beta2, float eps, float grad_scale, float l2,
                          chebgcn_stream stream);

/* ---- host-side index maps (no GPU): lib_new/coarsening.py -----------------------
 * metis_one_level (:120-166): one greedy matching pass, bit-exact incl. the
 * reference's row-length quirk.  rr/cc: int64 [nnz] sorted by rr; vv/weights in the
 * given precision; rid: int64 [N] visiting order; cluster_id: int32 [N] out.
 * The matching score vv*(1.0/weights[tid] + 1.0/weights[nid]) (:153) is evaluated as NumPy evaluates it
 * on scalars of that dtype: _f32 entirely in float32 (NumPy >= 2, NEP 50: a Python float does not widen
 * a float32 scalar), _f64 in float64, and _f32p on float32 inputs PROMOTED to float64 -- what NumPy 1.x
 * (the generation the reference was written for) does with a float32 graph; near-ties of the strict `>`
 * can fall differently between _f32 and _f32p (tests/golden/coarsen_unit_n*.npz holds both outcomes).
 * compute_perm (:168-215) for ONE level: children of `order` (length n_order) among
 * the fine vertices with `parent` (length n_fine); out must hold 2*n_order. */
int chebgcn_metis_one_level_f32(int64_t nnz, const int64_t* rr, const int64_t* cc, const float* vv,
                                const int64_t* rid, const float* weights, int64_t N, int32_t* cluster_id);
int chebgcn_metis_one_level_f32p(int64_t nnz, const int64_t* rr, const int64_t* cc, const float* vv,
                                 const int64_t* rid, const float* weights, int64_t N, int32_t* cluster_id);
int chebgcn_metis_one_level_f64(int64_t nnz, const int64_t* rr, const int64_t* cc, const double* vv,
                                const int64_t* rid, const double* weights, int64_t N, int32_t* cluster_id);
int chebgcn_compute_perm_level(const int32_t* parent, int64_t n_fine, const int64_t* order,
                               int64_t n_order, int64_t* out);


/* ---- spectral filters: filter = 'fourier' / 'spline' (lib_new/models_gcn.py:512-556) ---------------------------------
 * The graph Fourier basis U = the eigenvectors of the layer's Laplacian (lib_new/graph.py:110-128), U[vertex][frequency],
 * lives on the device as [Mp][Mp] fp32 with zero padding (Mp = chebgcn_plane_stride(M)).  Planes are [R][Mp] (R = B*F) in
 * the plane layout; the pad [M, Mp) of an input plane is never read, that of an output plane is written as 0.  Every sum
 * runs in a fixed order (no atomics): repeated calls are bit-identical.
 *
 * transform (fp32-input matrix instructions, exact fp32 products):
 *   transpose == 0 (analysis):  out[r][j] = sum_m in[r][m] * U[m][j]
 *   transpose != 0 (synthesis): out[r][j] = sum_m in[r][m] * U[j][m]
 * Not in place.  The gradient of either direction is the other one. */
int chebgcn_spectral_transform(const float* in, const float* basis, float* out, int R, int M, int transpose,
                               chebgcn_stream stream);
/* The per-frequency filter, W [M][Fout][Fin] row-major (the reference's weight shape), xh / dxh [B][Fin][Mp],
 * yh / dyh [B][Fout][Mp]:
 *   mix_fwd:   yh[b][o][m]    = sum_fin W[m][o][fin] * xh[b][fin][m]
 *   mix_bwd_x: dxh[b][fin][m] = sum_o   W[m][o][fin] * dyh[b][o][m]
 *   mix_bwd_w: dW[m][o][fin]  = sum_b dyh[b][o][m] * xh[b][fin][m]   (written, not accumulated) */
int chebgcn_spectral_mix_fwd(const float* xh, const float* W, float* yh, int B, int M, int Fin, int Fout,
                             chebgcn_stream stream);
int chebgcn_spectral_mix_bwd_x(const float* dyh, const float* W, float* dxh, int B, int M, int Fin, int Fout,
                               chebgcn_stream stream);
int chebgcn_spectral_mix_bwd_w(const float* dyh, const float* xh, float* dW, int B, int M, int Fin, int Fout,
                               chebgcn_stream stream);
/* Spline parametrisation of the filter (models_gcn.py:540-556): Bs [M][K] (the cubic B-spline basis at the eigenvalues),
 * Wk [K][C], W [M][C], C = Fout*Fin (column fout*Fin + fin):
 *   expand:     W[m][c]   = sum_k Bs[m][k] * Wk[k][c]
 *   expand_bwd: dWk[k][c] = sum_m Bs[m][k] * dW[m][c]   (written, not accumulated) */
int chebgcn_spectral_spline_expand(const float* Bs, const float* Wk, float* W, int M, int K, int C, chebgcn_stream stream);
int chebgcn_spectral_spline_expand_bwd(const float* Bs, const float* dW, float* dWk, int M, int K, int C,
                                       chebgcn_stream stream);

/* ---- saliency maps: input gradients and integrated gradients of a trained model (models_gcn.base_model.saliency) -------
 * The pass between these calls is the library's own forward (with ReLU masks) and the training step's input-gradient kernels.
 *
 * seed: the gradient of the attributed score wrt the logits, and the class it is attributed to.
 *   logits, dlogits: [B][C] dense; row r attributes targets[r / rep] (int64, device), or where targets is NULL the row's own
 *   first maximum (torch.argmax; a NaN counts as the largest value);  score CHEBGCN_SCORE_LOGIT: dlogits[r] = e_t,
 *   CHEBGCN_SCORE_LOGPROB (log softmax(z)_t): e_t - softmax(z_r).  Rows r >= nvalid get dlogits 0.  cls_out (int64, or NULL):
 *   cls_out[r / rep] = t for the rows r < nvalid with r % rep == 0.  dlogits may be NULL (the class alone).  A target outside
 *   [0, C) gives a NaN row.
 * path: the integrated-gradients path in plane storage.  x: [S][N][F] windows in row layout (device); perm: int32 [M] internal
 *   position -> vertex of x (NULL: identity, M == N); sample: int32 [nw] rows of x; baseline: [N][F] or NULL (zeros);
 *   out: [R][F][Mp(M)], R >= nw*steps:
 *     out[w*steps + j][f][i] = x0 + a_j (x[sample[w]][perm[i]][f] - x0),  x0 = baseline[perm[i]][f],  a_j = (j + 1/2) / steps
 *   rows from nw*steps and the pad [M, Mp) of every plane are 0.
 * reduce: dx: [nw*steps][F][Mp(M)] input-gradient planes (internal order, perm as above, M == N); the steps of a window are
 *   summed in order, g = sum_j dx[w*steps + j], and written in the caller's order to out [nw][M][F]:
 *     CHEBGCN_SAL_GRADIENT g,  CHEBGCN_SAL_GRAD_X_INPUT x g,  CHEBGCN_SAL_INTEGRATED (x - x0) g / steps   (x = x[sample[w]],
 *     x0 = baseline or 0), |.| when `absolute`.  With acc (float64 [ncls][M][F], device): acc[k] += the sum, windows in order,
 *   of out[w] over the windows with cls[w] == k (int64 [nw]; other values are skipped).  Fixed-order sums throughout. */
/* chebgcn_saliency_supported: 1 where path and reduce serve F channels (their LDS tiles: F <= 126), else 0.  Host only. */
enum { CHEBGCN_SCORE_LOGIT = 0, CHEBGCN_SCORE_LOGPROB = 1 };
int chebgcn_saliency_supported(int F);
enum { CHEBGCN_SAL_GRADIENT = 0, CHEBGCN_SAL_GRAD_X_INPUT = 1, CHEBGCN_SAL_INTEGRATED = 2 };
int chebgcn_saliency_seed(const float* logits, const int64_t* targets, int rep, int nvalid, int score, float* dlogits,
                          int64_t* cls_out, int B, int C, chebgcn_stream stream);
int chebgcn_saliency_path(const float* x, const int32_t* perm, const int32_t* sample, const float* baseline, float* out, int nw,
                          int steps, int R, int N, int M, int F, chebgcn_stream stream);
int chebgcn_saliency_reduce(const float* dx, const float* x, const int32_t* perm, const int32_t* sample, const float* baseline,
                            int nw, int steps, int M, int F, int method, int absolute, float* out, const int64_t* cls, int ncls,
                            double* acc, chebgcn_stream stream);

/* ---- occlusion maps: score drops when vertex groups are set to a baseline (models_gcn.base_model.occlusion) ------------
 * Rows are (window, group) pairs, window-major, G + 1 per window: row r is window w = r / (G + 1), slot j = r % (G + 1); slot 0
 * is the window itself (group g = G, which no vertex has), slot j >= 1 occludes group g = j - 1.  Between rows and score runs
 * the library's own forward.
 *
 * rows: rows r0 .. r0 + R - 1 in plane storage.  x: [S][N][F] windows in row layout (device); perm: int32 [M] internal position
 *   -> vertex of x (NULL: identity, M == N); gid: int32 [M] (or longer) group of each internal position, -1 = never occluded;
 *   baseline: [N][F] or NULL (zeros); out: [R][F][Mp(M)], 16-byte aligned:
 *     out[r - r0][f][i] = gid[i] == g_r ? baseline[perm[i]][f] : x[w_r][perm[i]][f]
 *   the pad [M, Mp) and the rows r >= S (G + 1) are 0.  R <= 65535.
 * score: logits [R][C] of rows r0 .. r0 + R - 1; cls: int64 [S] class of each window (a class outside [0, C) gives NaN);
 *   s = z_c (CHEBGCN_SCORE_LOGIT) or log softmax(z)_c (CHEBGCN_SCORE_LOGPROB, the maximum subtracted, classes summed in order).
 *   A slot-0 row writes ref[w] = s; a row of slot j >= 1 writes drop[w][j - 1] = s(slot 0 of w) - s, its slot-0 row read from
 *   logits when it lies in this call, else from ref[w] (written by an earlier call on the same stream).  ref: [S], drop: [S][G].
 * class_sums: acc[k][g] += the sum, windows in order, of drop[w][g] over the windows with cls[w] == k (float64 [ncls][G];
 *   other classes are skipped).  Fixed-order sums throughout; no atomics. */
/* chebgcn_occlusion_supported: 1 where the row kernel serves F channels (its LDS tiles: F <= 125), else 0.  Host only. */
int chebgcn_occlusion_supported(int F);
int chebgcn_occlusion_rows(const float* x, const int32_t* perm, const int32_t* gid, const float* baseline, float* out, int64_t r0,
                           int R, int S, int G, int N, int M, int F, chebgcn_stream stream);
int chebgcn_occlusion_score(const float* logits, int64_t r0, int R, int S, int G, int C, const int64_t* cls, int score, float* ref,
                            float* drop, chebgcn_stream stream);
int chebgcn_occlusion_class_sums(const float* drop, const int64_t* cls, int S, int G, int ncls, double* acc,
                                 chebgcn_stream stream);

/* ---- Shapley maps: sampled Shapley values of vertex groups (models_gcn.base_model.shapley) --------------------------------
 * A run has P permutations of the G groups, the same for every window, given as their inverse: rank: int32 [P][G] (device),
 * rank[p][g] = the position of group g in permutation p.  Rows are (window, permutation, prefix length) triples in that order,
 * P (G + 1) per window: row r is window w = r / (P (G + 1)), permutation p = (r / (G + 1)) % P, prefix length j = r % (G + 1);
 * it holds the window's own values on the first j groups of permutation p and the baseline on the others (j = 0: the baseline
 * window, j = G: the window itself).  P (G + 1) < 2^31.  Between rows and score runs the library's own forward.
 *
 * rows: rows r0 .. r0 + R - 1 in plane storage.  x, perm, baseline, out: as chebgcn_occlusion_rows; gid: int32 [M] (or longer)
 *   group of each internal position, a value outside [0, G) = outside the game (the position always keeps its own value):
 *     out[r - r0][f][i] = gid[i] outside [0, G) || rank[p_r][gid[i]] < j_r ? x[w_r][perm[i]][f] : baseline[perm[i]][f]
 *   the pad [M, Mp) and the rows r >= S P (G + 1) are 0.  R <= 65535.  A workgroup writes 16 consecutive rows of 64 positions
 *   and reads a window's tile once for all of them that belong to that window.
 * score: logits [R][C] of rows r0 .. r0 + R - 1 -> table[r] = s, the score table float32 [S][P][G + 1] that stays on the device
 *   for the run; s and cls as chebgcn_occlusion_score (a class outside [0, C) gives NaN).  Rows r >= S P (G + 1) write nothing.
 *   THE CLASS RULE: cls[w] must be final before the first row of window w is scored.  Under 'predicted' the caller therefore
 *   runs one plain forward over the windows first (chebgcn_saliency_seed's argmax); the row order is never rearranged.
 * reduce: once every row of the S windows is scored,
 *     phi[w][g] = (1/P) sum_p ( table[w][p][rank[p][g] + 1] - table[w][p][rank[p][g]] )        (float32 [S][G])
 *   the differences and their sum in float64, p ascending, one float64 division, one rounding to float32; one thread per
 *   (w, g).  A rank entry outside [0, G) gives NaN.  The per-class sums of phi are chebgcn_occlusion_class_sums.
 * Fixed-order sums throughout; no atomics. */
/* chebgcn_shapley_supported: 1 where the row kernel serves F channels (its LDS tiles: F <= 125), else 0.  Host only. */
int chebgcn_shapley_supported(int F);
int chebgcn_shapley_rows(const float* x, const int32_t* perm, const int32_t* gid, const int32_t* rank, const float* baseline,
                         float* out, int64_t r0, int R, int S, int P, int G, int N, int M, int F, chebgcn_stream stream);
int chebgcn_shapley_score(const float* logits, int64_t r0, int R, int S, int P, int G, int C, const int64_t* cls, int score,
                          float* table, chebgcn_stream stream);
int chebgcn_shapley_reduce(const float* table, const int32_t* rank, int S, int P, int G, float* phi, chebgcn_stream stream);

/* ---- Grad-CAM maps: class activation maps at a conv layer (models_gcn.base_model.gradcam) --------------------------------
 * A: the layer's activation, G = ds/dA its gradient (the library's input-gradient kernels, stopped at the layer); both plane
 * storage [>= nw][F][Mp(N)] over the N vertices of the layer's level in its internal order, 16-byte aligned.  Only the real
 * positions i < N are read (the pad may hold anything).  Fixed-order sums throughout; no atomics.
 *
 * weights: alpha[r][f] = (1/N) sum_{i<N} G[r][f][i] for the rows r < nw (float32 [nw][F]; the sum in float64, in order).
 * map: cam_i = sum_f alpha[r][f] A[r][f][i] (G NULL, alpha given: Grad-CAM) or sum_f G[r][f][i] A[r][f][i] (alpha NULL, G
 *   given: gradient x activation), filters in order, max(0, .) when relu != 0.  order: int32 [N] internal position -> reference
 *   vertex of the level (NULL: identity).  Reference vertex j covers the P (a power of two) input vertices [j P, (j + 1) P):
 *     out[r * ldo + j P + q] = cam_i,  j = order[i],  q < P,  r < nw  (ldo >= N P; nothing else is written). */
int chebgcn_gradcam_weights(const float* G, int nw, int F, int N, float* alpha, chebgcn_stream stream);
int chebgcn_gradcam_map(const float* A, const float* G, const float* alpha, const int32_t* order, int nw, int F, int N, int P,
                        int relu, float* out, int64_t ldo, chebgcn_stream stream);

/* ---- training on scans: a dataset that IS windows of scans (models_gcn.base_model.stage_windows / fit_series) --------------
 * series: [Ttot][Mp(M)] planes, every run of the dataset concatenated, in the model's internal vertex order, zero in the pad
 * (what decode_series stages); rows: int64 [.] on the device, the global row of each window's first time point (run offset +
 * start).  Window w is the model input x[w][c][m] = series[rows[w] + c][m], c < C: C consecutive planes, never stored per window.
 * Every row must satisfy 0 <= row and row + C <= Ttot: the CALLER checks the table before it uploads it; a row outside that
 * range is moved into it by the kernels (the rule of chebgcn_contract_fwd_windows), which never read outside the series.
 *
 * gather_windows: out[b][c][m] = series[rows[sample[b]] + c][m], [B][C][Mp]; sample: int32 [B] (device) indices into rows, or
 *   NULL for the identity (as chebgcn_perm_data).  With scale / shift ([C][Mp], both or neither):  x * scale + shift  as a
 *   rounded product followed by a rounded sum (never one fma: bit-identical to float32 NumPy).  The pad [M, Mp) of every
 *   output plane is written as 0.  Bit-identical to chebgcn_perm_data on the windows cut on the host.  16-byte accesses;
 *   series, tables and out 16-byte aligned; B <= 65535.  chebgcn_last_dispatch(): gather_windows_kernel<plain | tables>.
 * gather_windows_mix: a window that is the MEAN of several source windows (class balancing, series.balance_plan).  rows: int64
 *   [.][smax], cnt: int32 [.] (device), 1 <= smax <= 16; with w = sample ? sample[b] : b and n = cnt[w]
 *     out[b][c][m] = ( sum_{j < n} series[rows[w][j] + c][m] ) / n     (then * scale[c][m] + shift[c][m], as above).
 *   The sum is formed in float32 in ascending j, followed by ONE correctly rounded float32 division by (float)n, then the
 *   rounded product and the rounded sum of the tables: every result is reproducible bit for bit in float32 NumPy, and a window
 *   with n == 1 is bit-identical to gather_windows on rows[w][0].  A count outside [1, smax] is clamped into it (it is never a
 *   trip count taken from memory unchecked); every row is clamped like gather_windows' rows.  Pad, alignment and B as
 *   gather_windows.  Traffic: (n + 1) windows per output window.  chebgcn_last_dispatch():
 *   gather_windows_mix_kernel<plain | tables>.
 * window_stats: mean[c][m] and population variance var[c][m] (ddof = 0, sklearn's StandardScaler) of x[w][c][m] over the S
 *   windows rows[0 .. S), float64 [C][Mp] (either may be NULL), and the float32 tables scale = 1/std, shift = -mean/std
 *   ([C][Mp]; where the variance is 0: scale 1, shift -mean; the pad of all four is 0).  One pass over the series whatever the
 *   overlap (a per-row count of the windows that start there, then  sum_u n[u - c] f(series[u][m])).  Float64 sums of the
 *   deviations from series[0][m] in ascending row order inside chunks of 512 rows, chunks added in index order, every sum
 *   carried as a pair of doubles (head + tail: no rounding of a sum or of a square reaches the variance, which is 0 for one
 *   window): no float atomics, bit-identical from run to run and under any permutation of rows.  workspace: device scratch of
 *   at least chebgcn_window_stats_workspace() bytes, 16-byte aligned.  chebgcn_last_dispatch(): window_count_kernel +
 *   window_stats_partial_kernel + window_stats_finish_kernel.
 *
 * Windows that are LISTS of rows (events.match_events: a trial padded by repeating its last volume, a chunk that straddles a rest
 * period, the mean of TRstep sub-windows).  idx: int64 [S][Cin] (device), Cin = C * fold, rows of the concatenated planes;
 * channel c of window s is the mean of the fold rows idx[s][f * C + c], f < fold:
 *     piece(s)[c][m] = ( series[idx[s][0 * C + c]][m] + ... + series[idx[s][(fold - 1) * C + c]][m] ) / fold.
 * gather_windows_indexed: src int64 [W][smax] with cnt int32 [W] (both or neither; series.balance_plan's indices INTO idx,
 *   1 <= smax <= 16; NULL: every window is its own single source and W is ignored).  With w = sample ? sample[b] : b,
 *   n = cnt[w] (1 without src):
 *     out[b][c][m] = ( piece(src[w][0]) + ... + piece(src[w][n - 1]) ) / n     (then * scale[c][m] + shift[c][m]).
 *   Float32 adds (round to nearest) in ascending order at both levels; each level takes ONE correctly rounded division, and
 *   only when its count is above 1; the tables apply as a rounded product followed by a rounded sum, never one fma: bit for
 *   bit reproducible in float32 NumPy, equal to gather_windows on contiguous rows at fold = 1 without src, and to
 *   gather_windows_mix with src.  fold must lie in [1, 16] (and Cin == C * fold); n is clamped into [1, smax]; w is clamped
 *   into [0, W - 1] (without src: [0, S - 1]), every entry of src into [0, S - 1] and every row into [0, Ttot - 1]: nothing
 *   read from memory is an address or a trip count unchecked.  Pad, alignment and B as gather_windows.  Traffic:
 *   (fold * n + 1) windows per output window.  chebgcn_last_dispatch(): gather_windows_indexed_kernel<plain | tables>.
 * window_stats_indexed: what window_stats computes, over piece(s), s < S -- the folded values as the gather forms them in
 *   float32, before the tables and without sources (what the reference's scaler sees, utils.py:573).  Float64 sums of the
 *   deviations from series[0][m], as pairs of doubles like window_stats'; one workgroup sums a chunk of windows in ascending
 *   order (chunks of max(16, ceil(S / 32)) windows), chunks are added in index order: no float atomics, bit-identical from run
 *   to run.  workspace: at least
 *   chebgcn_window_stats_indexed_workspace() bytes, 16-byte aligned.  chebgcn_last_dispatch():
 *   window_stats_indexed_partial_kernel + window_stats_finish_kernel. */
int chebgcn_gather_windows(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* sample, const float* scale,
                           const float* shift, float* out, int B, int M, int C, chebgcn_stream stream);
int chebgcn_gather_windows_mix(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* cnt, int smax,
                               const int32_t* sample, const float* scale, const float* shift, float* out, int B, int M, int C,
                               chebgcn_stream stream);
size_t chebgcn_window_stats_workspace(int64_t Ttot, int M, int C);
int chebgcn_window_stats(const float* series, int64_t Ttot, const int64_t* rows, int64_t S, double* mean, double* var,
                         float* scale, float* shift, int M, int C, void* workspace, size_t workspace_bytes,
                         chebgcn_stream stream);
int chebgcn_gather_windows_indexed(const float* series, int64_t Ttot, const int64_t* idx, int64_t S, int Cin, int fold,
                                   const int64_t* src, const int32_t* cnt, int64_t W, int smax, const int32_t* sample,
                                   const float* scale, const float* shift, float* out, int B, int M, int C,
                                   chebgcn_stream stream);
size_t chebgcn_window_stats_indexed_workspace(int64_t S, int M, int C);
int chebgcn_window_stats_indexed(const float* series, int64_t Ttot, const int64_t* idx, int64_t S, int Cin, int fold,
                                 double* mean, double* var, float* scale, float* shift, int M, int C, void* workspace,
                                 size_t workspace_bytes, chebgcn_stream stream);

/* ---- augmented training windows (series.WindowSet.augment): vertex dropout and time shifts, copy by copy, never stored --------
 * An augmented set stands for copies * S windows; augmented window i is base window i % S, copy i / S.  What perturbs window i
 * is a stateless function of (seed, refill, i, d) -- never of the batch the window lands in or of its place there:
 *
 *   fin(x):  x ^= x >> 16;  x *= CHEBGCN_AUG_MUL1;  x ^= x >> 15;  x *= CHEBGCN_AUG_MUL2;  x ^= x >> 16     (uint32, wrapping)
 *   a  = fin(fin(seed) + refill)
 *   k0 = fin(a + i)
 *   k1 = fin((a ^ CHEBGCN_AUG_KEY) + i * CHEBGCN_AUG_WINDOW)
 *   chebgcn_aug_draw(seed, refill, i, d) = fin(fin(k0 + d) ^ k1)                                  (32 uniform bits)
 *   a value u becomes an integer of [0, n) as ((uint64_t)u * n) >> 32, without a modulo.
 * For fixed (seed, refill), i -> (k0, k1) is one to one: no two windows of a refill share their stream.  Draws d = 0 .. D - 1 of
 * window i are its dropped vertices (out of [0, M), with replacement); draw d = CHEBGCN_AUG_SHIFT_DRAW is its time shift (out of
 * [0, C)).  series.drop_vertices / series.time_shifts restate both in NumPy.
 *
 * window_drop: in place on a gathered batch x [B][C][Mp(M)].  win: int32 [B] (device), the augmented-set index i of every batch
 *   row; pos: int32 [M] (device), vertex in the caller's order -> position in the batch's vertex order, NULL: the identity.  For
 *   every b < B and d < D, with v = the draw (seed, refill, win[b], d) in [0, M) and p = pos[v]:
 *     x[b][c][p] = drop_value                                   for every c < C, or, with scale / shift ([C][Mp], both or neither),
 *     x[b][c][p] = drop_value * scale[c][p] + shift[c][p]       as a rounded product followed by a rounded sum (never one fma):
 *   the value the gathers would have stored had the series held drop_value there.  Nothing else is written -- B * D * C * 4
 *   bytes per batch, the pad included in "nothing else".  Draws that repeat a vertex store the same value twice: no atomics, the
 *   result does not depend on the order of the stores.  win[b] enters the generator only; pos[v] is clamped into [0, M - 1]
 *   before it is an address.  D may exceed M.  D == 0 or B == 0: no launch (chebgcn_last_dispatch(): "").  B * D <= 2^31 * 256.
 *   chebgcn_last_dispatch(): window_drop_kernel<plain | tables>.
 * gather_windows_reflect: chebgcn_gather_windows with a time shift per window.  tshift: int32 [.] (device) indexed like rows;
 *   with w = sample ? sample[b] : b, r = tshift[w] clamped into [0, C - 1] (NULL: 0) and
 *   rho(j) = j for j < C, 2 C - 1 - j otherwise:
 *     out[b][c][m] = series[rows[w] + rho(c + r)][m]            (then * scale[c][m] + shift[c][m]: the tables of OUTPUT channel c)
 *   -- numpy.pad(x, C, 'symmetric')[r + C : r + 2 C] along the channels of window x.  Rows are clamped as gather_windows
 *   clamps them; pad, alignment and B as there; bit-identical to gather_windows where tshift is NULL or all zero.
 *   chebgcn_last_dispatch(): gather_windows_reflect_kernel<plain | tables>. */
#define CHEBGCN_AUG_MUL1 0x7FEB352Du
#define CHEBGCN_AUG_MUL2 0x846CA68Bu
#define CHEBGCN_AUG_KEY 0x9E3779B9u
#define CHEBGCN_AUG_WINDOW 0x85EBCA6Bu
#define CHEBGCN_AUG_SHIFT_DRAW 0xFFFFFFFFu
int chebgcn_window_drop(float* x, const int32_t* win, int B, int M, int C, int D, uint32_t seed, uint32_t refill,
                        const int32_t* pos, const float* scale, const float* shift, float drop_value, chebgcn_stream stream);
int chebgcn_gather_windows_reflect(const float* series, int64_t Ttot, const int64_t* rows, const int32_t* tshift,
                                   const int32_t* sample, const float* scale, const float* shift, float* out, int B, int M, int C,
                                   chebgcn_stream stream);

/* ---- Monte-Carlo dropout: S stochastic passes of the head from one pass of the trunk (models_gcn.base_model.predict_mc) ----------
 * Dropout exists only behind the hidden FC layers of the head (tf.nn.dropout, models_gcn.py:674-682): dropout site j (0-based)
 * follows fc{j+1}.  The mask is a pure function of (seed, sample, site, window, feature) on the generator above:
 *     u    = chebgcn_aug_draw(seed, refill = sample * CHEBGCN_MC_SITES + site, i = window, d = feature)
 *     kept = u < T,   T = min((uint64_t)(keep * 2^32), 2^32 - 1)   (computed by the CALLER from the float64 keep, passed as uint32)
 *     value = kept ? x * inv_keep : +0,   inv_keep = (float)(1 / keep), ONE rounded float32 product (never part of an fma)
 * `window` is the index of the window in the caller's data, never its place in a batch: results do not depend on the batching.
 * uncertainty.dropout_keep restates the mask in NumPy.  No mask is ever stored.
 *
 * fc_fwd_dropout: chebgcn_fc_fwd for S samples of one layer,
 *     y[s][b][o] = act( sum_{i<I} value(s0 + s, layer, win[b], i; x_s[b][i]) * W[i][o] + bias[o] ),   s < S, y float32 [S][B][O]
 *   x_s = x + s * sample_stride, B rows of row stride ldx >= I each (elements; 16-byte aligned, ldx and sample_stride multiples
 *   of 4, whole rows readable: chebgcn_fc_fwd's rules; values past I in a row never reach the product).  sample_stride == 0: one
 *   [B][ldx] matrix shared by every sample (the first site: fc1's output is computed once); else >= (B - 1) * ldx + I.  win: int32
 *   [B] (device), the window number of every row; it enters the generator as a uint32 and is never an address.  s0 >= 0: the
 *   number of the launch's first sample (callers send S samples in chunks); 0 <= layer < CHEBGCN_MC_SITES.  The tiling, the
 *   order of every sum and the split of the reduction across workgroups are chebgcn_fc_fwd's (the splits count the tiles of all S
 *   samples): deterministic, no atomics.  Served: chebgcn_fc_fwd_dropout_supported -- I <= 2^20, S * B * O <= 2^20 per launch,
 *   S <= 32768; CHEBGCN_EUNSUPPORTED beyond, or for an unaligned x / ldx / sample_stride.  workspace: at least
 *   chebgcn_fc_fwd_dropout_workspace() bytes of device scratch (0: none needed).  chebgcn_last_dispatch():
 *   fc_fwd_dropout_kernel<shared | per_sample>, or fc_fwd_dropout_kernel<shared | per_sample, split> + fc_fwd_reduce_kernel.
 * mc_reduce: logits float32 [S][B][C] -> per window b, with p_s = softmax(logits[s][b]) (maximum subtracted) and
 *   H(p) = -sum_c p_c log p_c in nats, 0 log 0 = 0:
 *     mean_p[b][c]           = (sum_s p_s[c]) / S        (float32 [B][C]; the sum in sample order, one division)
 *     entropy[b]             = H(mean_p)
 *     expected_entropy[b]    = (sum_s H(p_s)) / S
 *     mutual_information[b]  = max(0, entropy - expected_entropy)   (>= 0 in exact arithmetic; the two sums are rounded apart)
 *     label[b]               = the first maximum of mean_p[b]        (int32)
 *     votes[b][c]            = #{s : c is the first maximum of logits[s][b]}, a NaN counting as the largest value
 *                              (chebgcn_saliency_seed's rule; int32 [B][C])
 *     agreement[b]           = votes[b][label[b]] / S
 *   Never NaN for finite logits (saturated softmaxes included).  One wave per window; fixed-order sums (float64 over the samples),
 *   no atomics: reruns are bit-identical.  Served: chebgcn_mc_reduce_supported -- 1 <= C <= 64, 1 <= S <= 1024;
 *   CHEBGCN_EUNSUPPORTED beyond, before any launch.  chebgcn_last_dispatch(): mc_reduce_kernel. */
#define CHEBGCN_MC_SITES 16
int chebgcn_fc_fwd_dropout_supported(int S, int B, int I, int O);
size_t chebgcn_fc_fwd_dropout_workspace(int S, int B, int I, int O);
int chebgcn_fc_fwd_dropout(const float* x, int64_t ldx, int64_t sample_stride, const float* W, const float* bias, float* y,
                           void* workspace, size_t workspace_bytes, const int32_t* win, int S, int B, int I, int O, int relu,
                           uint32_t seed, int s0, int layer, uint32_t threshold, float inv_keep, chebgcn_stream stream);
int chebgcn_mc_reduce_supported(int S, int C);
int chebgcn_mc_reduce(const float* logits, int S, int B, int C, float* mean_p, float* entropy, float* expected_entropy,
                      float* mutual_information, int32_t* label, int32_t* votes, float* agreement, chebgcn_stream stream);

/* ---- kNN brain graphs on the device (graph.knn_device / graph.connectivity_graph) ------------------------------------------
 * feat: [D][Np(N)] fp32, feature-major planes of N vertices (the staged-series layout with D = time; coordinates are
 * transposed by the caller), zero in the pad.  For every vertex i the k nearest OTHER vertices under `metric`:
 *   dist: float32 [N][k] ascending;  idx: int32 [N][k].  Vertex i itself is excluded BY INDEX (the reference drops column 0 of
 *   the sorted row instead, graph.py:14: where points coincide that can drop another vertex and keep i as its own neighbour at
 *   distance 0; everywhere else the two agree).  Equal distances order by lower index first.
 *   EUCLIDEAN    |a - b|
 *   COSINE       1 - a.b / (|a| |b|)
 *   CORRELATION  cosine of the rows centred over d
 *   DOT          1 - a.b, rows taken as prepared by the caller (the output of chebgcn_series_normalise with scale =
 *                1/sqrt(R): 1 - the mean over runs of the per-run Pearson correlation)
 *                (arms by D like every metric: a series of at most 8 time points in all runs the direct arm)
 *   A zero-norm row under COSINE and a constant row under CORRELATION have similarity 0 (distance 1) to everything: never NaN.
 *   Features must be finite (the caller checks).
 * Served: 1 <= k <= 32 (CHEBGCN_EUNSUPPORTED beyond) and k < N (CHEBGCN_EINVAL), checked before any launch.
 * Arms (chebgcn_last_dispatch(): knn_prep_kernel + <arm> + knn_merge_refine_kernel):
 *   knn_direct_kernel<whole | split>  D <= 8: differences / products on the vector ALU, a thread per query;
 *   knn_gram_kernel<whole | split>    D > 8: the Gram tile on v_mfma_f32_32x32x2_f32 (any D: odd, not a multiple of the
 *                                     eight-feature loop turn), a wave per 32 queries, lists of candidates in LDS;
 *   <split>: fewer query blocks than CUs, the candidate range is cut into up to 8 pieces with their own partial lists.
 * Selection runs on float32 keys with k + 8 candidates kept per query; the k returned distances are recomputed from the
 * features with float64 accumulators in ascending d (never the cancelling Gram form) and rounded once to float32.  Prep sums
 * (means, norms) are float64 in ascending d.  No float atomics, every order fixed: two calls give bit-identical outputs.
 * workspace: device scratch of at least chebgcn_knn_workspace() bytes (0 = shape not served), 16-byte aligned, as is feat.
 *
 * series_normalise: series [Ttot][Mp(M)] = R runs concatenated, run r = rows [run_offsets[r], run_offsets[r + 1]) (int64
 *   [R + 1] on the device, ascending, run_offsets[R] = Ttot: the CALLER checks the table).  out[t][m] = (series[t][m] - mean)
 *   / norm * scale, mean and norm of vertex m inside ITS run (float64, ascending t); a vertex constant in a run is all zeros
 *   there, the pad is zero.  With scale = 1 the Gram matrix of out over t, divided by R, is the mean over runs of the per-run
 *   Pearson correlation matrices; neither is ever formed.  chebgcn_last_dispatch(): series_normalise_kernel. */
enum {
    CHEBGCN_KNN_EUCLIDEAN = 0,
    CHEBGCN_KNN_COSINE = 1,
    CHEBGCN_KNN_CORRELATION = 2,
    CHEBGCN_KNN_DOT = 3
};
size_t chebgcn_knn_workspace(int N, int D, int k);
int chebgcn_knn(const float* feat, int N, int D, int k, int metric, float* dist_out, int32_t* idx_out, void* workspace,
                size_t workspace_bytes, chebgcn_stream stream);
int chebgcn_series_normalise(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, float scale,
                             float* out, chebgcn_stream stream);

/* ---- parcellation: vertex-level scans reduced to atlas regions, and back (parcellation.Parcellation) --------------------------
 * parcellate: x float32, T rows of V values with row stride ldx >= V (elements; the offset t * ldx is 64-bit), vertex fastest;
 *   the member lists of the R regions in CSR form, ptr int32 [R + 1] and idx int32 [nnz] (device), members ASCENDING inside a
 *   region, every vertex at most once (nnz <= V); w float32 [V] per-vertex weights or NULL.  out float32 [T][R], row stride ldo.
 *     MEAN  out[t][r] = (sum_j x[t][idx[j]]) / n_r              with w:  (sum_j w[idx[j]] * x[t][idx[j]]) / (sum_j w[idx[j]])
 *     SUM   the numerator alone.
 *   Float32 throughout, round to nearest: acc = 0, then acc = acc + term for j = ptr[r], ptr[r] + 1, ... one after the other
 *   (a weighted term is a product rounded on its own, never an fma), the denominator of the weighted mean summed in the same
 *   order, ONE correctly rounded division at the end.  The order is a function of (ptr, idx) alone -- not of T, of the row a
 *   value stands in, of the launch geometry or of how the caller cuts the rows into calls: bit for bit reproducible in float32
 *   NumPy (parcellation.Parcellation.reduce_host) and from call to call.  No float atomics.  A region without members gives
 *   0 (SUM) or NaN (MEAN); a non-finite value reaches its own (t, r) only.  The lists are trusted (the caller checks them);
 *   an entry that does not ascend is skipped, ptr is clamped into [0, nnz]: nothing read from memory is an address unchecked.
 *   R <= 65535, V <= 2^30; x, w, out 4-byte aligned (any ldx: a row need not start on 16 bytes).  R above the regions of one
 *   pass (chebgcn_parcellate_query(3)) sweeps x once per pass.
 *   chebgcn_last_dispatch(): parcellate_kernel<rows1 | rows4, plain | weighted> -- rows4 (a workgroup owns 4 rows) from
 *   T >= chebgcn_parcellate_query(2) rows, rows1 below (more workgroups).
 * parcel_expand: out[b][v] = maps[b][region_of[v]], or `fill` where region_of[v] is outside [0, R) (-1: background); maps
 *   float32 [B][R], region_of int32 [V] (16-byte aligned), out float32 [B][V], all contiguous.
 *   chebgcn_last_dispatch(): parcel_expand_kernel.
 * parcellate_query: constants of the kernels, for callers and tests that must follow the tile -- 0 floats of x a workgroup holds
 *   per chunk (a chunk is that many / row tile vertices), 1 the row tile of rows4, 2 the rows from which rows4 runs, 3 regions
 *   per pass, 4 most workgroups of a parcellate launch (beyond: a workgroup loops), 5 most map rows of an expand grid, 6
 *   vertices per thread of expand; -1 for anything else. */
enum {
    CHEBGCN_PARCEL_MEAN = 0,
    CHEBGCN_PARCEL_SUM = 1
};
int chebgcn_parcellate_query(int what);
int chebgcn_parcellate(const float* x, int64_t ldx, const int32_t* ptr, const int32_t* idx, int64_t nnz, const float* w, float* out,
                       int64_t ldo, int64_t T, int V, int R, int mode, chebgcn_stream stream);
int chebgcn_parcel_expand(const float* maps, const int32_t* region_of, float* out, int64_t B, int R, int V, float fill,
                          chebgcn_stream stream);

/* ---- graph filters: y = h(L) x with fixed Chebyshev coefficients (filters.GraphFilter) ------------------------------------------
 * For every filter j < J and plane p < nplanes
 *     y[j][p] = sum_{k<K} coeff[j][k] * T_k(L~) x[p],    T_0 = x, T_1 = L~ x, T_k = 2 L~ T_{k-1} - T_{k-2},
 * summed in ascending k: coeff[j][0] * x as a rounded product, then one fmaf per order.  x: [nplanes][Mp]; coeff: float32 [J][K]
 * in DEVICE memory (a call uploads nothing); y: [J][nplanes][Mp].  x is never written; y may not overlap x; the pad [M, Mp) of
 * every plane of y and of the workspace is scratch (it may be written, it never reaches [0, M)).  The call does not synchronise
 * and does not allocate.  1 <= J <= 8, 1 <= K <= 256, 1 <= nplanes < 2^30; x, y and workspace 16-byte aligned.
 * arm: 0 automatic, 1 rolling, 2 stack.
 *   rolling  one launch of cheb_filter_step_kernel<P> per order (K == 1: one scale pass of the same kernel, no gather).  A thread
 *            owns one row of L~ for P consecutive planes (P = 4 from nplanes >= 4, the last group guarded; else 1), sums the row
 *            as one fmaf chain in the order of the CSR the handle was created from, stores T_k over T_{k-2} and adds it into the
 *            J accumulators.  Workspace: TWO slabs, 2 * nplanes * Mp * 4 bytes, whatever K and J.  Any graph; any nplanes in
 *            range (plane groups beyond the grid are looped over).  A plane's result is a function of that plane alone:
 *            bit-identical alone or among others, and from run to run.
 *   stack    the dispatch of chebgcn_recurrence_fwd into a workspace of K slabs, then one streaming launch of
 *            cheb_filter_mix_kernel (16-byte accesses, every stack element read once for all J filters).  Needs a handle with an
 *            on-chip or ordered image (chebgcn_graph_query 3 or 12), CHEBGCN_EUNSUPPORTED otherwise; K == 1 mixes x directly.
 *   automatic: stack when the handle has such an image and K > 1, rolling otherwise.
 * The arms differ in the order inside a row sum of L~ and agree to fp32 round-off, not bit for bit.
 * chebgcn_cheb_filter_workspace: bytes of the arm the call would take (0 for a NULL handle or arguments out of range).
 * chebgcn_last_dispatch(): cheb_filter_step_kernel<4 | 1>, or <the recurrence kernel> + cheb_filter_mix_kernel. */
size_t chebgcn_cheb_filter_workspace(const chebgcn_graph* g, int nplanes, int K, int J, int arm);
int chebgcn_cheb_filter(const chebgcn_graph* g, const float* x, const float* coeff, float* y, void* workspace, int nplanes, int K,
                        int J, int arm, chebgcn_stream stream);

/* ---- permutation inference on maps: sign-flip t maps and cluster enhancement on the graph (stats.map_test) ----------------------
 * signflip_t: x float32 [S][M] (one map per subject, contiguous), q float64 [M] (q[v] = sum_j x[j][v]^2, ascending j, computed
 *   once by the caller) -> t float32 [Pb][M], the one-sample t map of the permutations p0 .. p0 + Pb - 1.  Subject j of
 *   permutation p is negated where bit (j & 31) of bits[p - p0][j >> 5] is set (bits: uint32 [Pb][(S + 31) / 32], device), or,
 *   with bits == NULL, where the top bit of chebgcn_aug_draw(seed, refill = 0, i = p, d = j) is set; permutation 0 is then the
 *   identity.  Per (permutation, vertex), in float64, every operation rounded on its own (never an fma):
 *     s = 0;  s = s + (+-x[j][v])  for j = 0 .. S - 1;     m = s / S;     d = q[v] - s * m;
 *     t = d > 0 ? (float)(m / sqrt(d / (S * (S - 1)))) : 0         (one rounding to float32; a constant vertex gives 0)
 *   division and square root correctly rounded: bit for bit what float64 NumPy gives (stats.map_test_host).
 *   2 <= S <= 4096, M <= 2^24, Pb <= 65535: CHEBGCN_EUNSUPPORTED beyond, before any launch.  chebgcn_last_dispatch():
 *   signflip_t_kernel.
 * cluster_enhance: t float32 [Pb][M]; u = negate ? -t : t.  ptr int32 [M + 1] / idx int32 [nnz]: the graph's neighbour lists in
 *   CSR form (device; symmetric, no diagonal: the caller builds them; idx may be NULL when nnz == 0; an entry outside [0, M) is
 *   skipped, ptr is clamped into [0, nnz]).  Per permutation, with the caller's tables hf float32 [NH + 1] (heights, ASCENDING in i, entry 0 unused), hw
 *   float64 [NH + 1] and ep float64 [M + 1] (all device):
 *     MAX     out[p][v] = (double)u[v]; no graph, no tables, no status.
 *     TFCE    n = u_max > 0 ? floor((double)u_max / step) : 0 heights; vertex v is active at height i <= n when u[v] > hf[i];
 *             e_i(v) = the size of v's connected component among the active vertices;
 *             out[p][v] = sum over the heights i = n, n - 1, .. 1 at which v is active, IN THAT ORDER, of ep[e_i(v)] * hw[i]:
 *             acc = 0, acc = acc + (ep * hw), the product rounded, then the sum (float64).  No pow on the device.
 *     EXTENT  the same with n = 1 whatever u_max (hf[1] = the forming threshold; ep[e] = e and hw[1] = 1 give the extent).
 *   out float64 [Pb][M] or NULL; labels int32 [Pb][M] or NULL: the smallest vertex of v's component at height 1, -1 where v is
 *   not active there; pmax float64 [Pb] or NULL: max_v out[p][v].  At least one of the three.
 *   status: int32 [1] (device), zeroed by the caller.  The call does not synchronise and does not allocate; what only the device
 *   can find out is reported there and the caller reads it with the result: CHEBGCN_CLUSTER_EHEIGHTS = a permutation has more
 *   than NH heights, CHEBGCN_CLUSTER_ELOOP = a union-find loop ran past its bound of M turns.  Non-zero: the outputs are void.
 *   Labelling is a lock-free union-find (smaller root wins: compare-and-swap hooking, path halving); no workgroup waits for
 *   another; sizes are integer atomics; no float atomics: outputs are bit for bit reproducible and equal to the host restatement.
 *   Arms (arm: 0 automatic, 1 on chip, 2 streamed):
 *     on chip   M <= chebgcn_cluster_query(0): one workgroup takes one permutation through all heights with its state in LDS
 *               (chebgcn_cluster_query(5) bytes a vertex); no workspace.  chebgcn_last_dispatch(): cluster_onchip_kernel.
 *     streamed  any M: the state in `workspace` (chebgcn_cluster_enhance_workspace bytes, 16-byte aligned), NH heights of four
 *               launches each whatever the permutations need (EXTENT: one).  chebgcn_last_dispatch(): cluster_prep_kernel +
 *               cluster_hook_kernel + cluster_flatten_kernel + cluster_count_kernel + cluster_accum_kernel +
 *               cluster_final_kernel<state>.
 *     MAX runs cluster_final_kernel<plain> alone.
 *   Both arms give identical outputs.  M <= 2^24, Pb <= 65535, NH <= 65536: CHEBGCN_EUNSUPPORTED beyond (and for arm 1 above
 *   its limit), before any launch.
 * cluster_query: 0 vertices of the on-chip arm at most, 1 subjects, 2 vertices, 3 heights, 4 permutations of a call at most,
 *   5 bytes of state per (permutation, vertex); -1 for anything else.
 * cluster_enhance_workspace: bytes the call would take (0: the on-chip arm, MAX, or arguments out of range).
 * perm_glm_t: the t map of ONE contrast of a general linear model whose design is permuted (stats.design_test, the Freedman-Lane
 *   scheme).  The caller factors the design on the host, D = U S V^T (thin SVD, rank r), and hands the kernel
 *     e      float32 [S][M]   the residuals of the nuisance fit, one row per subject (contiguous; M is any number)
 *     q      float64 [M]      q[v] = sum_j e[j][v]^2, ascending j, computed once by the caller
 *     Uf     float64 [S][r]   = U[:, :r], row-major (device)
 *     u      float64 [r]      = Uf^T (pinv(D)^T c) (device);  unorm2 = c pinv(D^T D) c > 0 and dof = S - r >= 1 by value
 *     rows   uint32 [Pb][S]   (device) entry [p][j]: low 31 bits = the row of Uf that meets subject j in permutation p, top bit =
 *                             e[j] is negated.  A row number >= S is clamped to S - 1: it is never an address unchecked.
 *   -> t float32 [Pb][M], the layout cluster_enhance takes.  Per (permutation p, vertex v), in float64, every multiply, add,
 *   divide and square root rounded on its own (never an fma), division and square root correctly rounded:
 *     a_k = 0;  a_k = a_k + Uf[row(p, j)][k] * (+-e[j][v])   for j = 0 .. S - 1 ascending,   k = 0 .. r - 1
 *     ssq = 0;  ssq = ssq + a_k * a_k   k ascending;         num = 0;  num = num + u[k] * a_k   k ascending
 *     rss = q[v] - ssq, taken as 0 where rss < (4 (S + r) 2^-53) q[v]          (the floor glm_finish uses)
 *     var = (rss / dof) * unorm2;       t = var > 0 ? (float)(num / sqrt(var)) : 0
 *   bit for bit what float64 NumPy gives (stats.perm_t_host), and for a (p, v) the same bits whatever Pb, M or the rest of the
 *   table holds.  A workgroup takes chebgcn_perm_glm_query(0) vertices and (100 + r) permutations; r > (2) runs in column panels
 *   of (2) with e re-read per panel, ssq and num carried across them.  No synchronisation, no allocation, no atomics.
 *   2 <= S <= 4096, M <= 2^24, Pb <= 65535, r <= 64: CHEBGCN_EUNSUPPORTED beyond, before any launch; r >= S, dof < 1 or
 *   unorm2 <= 0: CHEBGCN_EINVAL.  chebgcn_last_dispatch(): perm_glm_t_kernel<n, one | panels>, n = the columns of the last (or
 *   only) panel.
 * perm_glm_query: 0 vertices of a workgroup, 1 permutations of a workgroup at most, 2 columns of a panel, 3 rank, 4 subjects,
 *   5 vertices, 6 permutations of a call at most, 100 + r (r = 1 .. 64) permutations of a workgroup at rank r; -1 for anything
 *   else. */
enum {
    CHEBGCN_CLUSTER_MAX = 0,
    CHEBGCN_CLUSTER_EXTENT = 1,
    CHEBGCN_CLUSTER_TFCE = 2
};
enum {
    CHEBGCN_CLUSTER_EHEIGHTS = 1,
    CHEBGCN_CLUSTER_ELOOP = 2
};
int chebgcn_cluster_query(int what);
size_t chebgcn_cluster_enhance_workspace(int Pb, int M, int mode, int arm);
int chebgcn_signflip_t(const float* x, const double* q, const uint32_t* bits, float* t, int S, int M, uint32_t p0, int Pb,
                       uint32_t seed, chebgcn_stream stream);
int chebgcn_perm_glm_query(int what);
int chebgcn_perm_glm_t(const float* e, const double* q, const double* Uf, const double* u, double unorm2, int dof,
                       const uint32_t* rows, float* t, int S, int M, int r, int Pb, chebgcn_stream stream);
int chebgcn_cluster_enhance(const int32_t* ptr, const int32_t* idx, int64_t nnz, const float* t, int negate, const float* hf,
                            const double* hw, int NH, const double* ep, double step, double* out, int32_t* labels, double* pmax,
                            int32_t* status, void* workspace, size_t workspace_bytes, int Pb, int M, int mode, int arm,
                            chebgcn_stream stream);

/* ---- first-level GLM on staged scans: projections, residual variance, contrasts (glm.first_level) ------------------------------
 * The caller factors every run's design on the host, X = U S V^T (thin SVD, rank k_r), and hands the kernels
 *   Q = U[:, :k_r]                        float64 [Ttot][k]: row t belongs to the run that contains t; columns [k_r, k) are zero
 *   u = (V[:, :k_r] / S[:k_r])^T c        float64 [R][C][k] per contrast c, and unorm2 = u.u = c pinv(X^T X) c, float64 [R][C]
 *   B = V[:, :k_r] / S[:k_r]              float64 [R][P][k] (b = B a is the minimum-norm solution), only for the coefficients
 *   rank[r] = k_r                         int32 [R]
 * series: float32 [Ttot][Mp(M)] = R runs concatenated, run r = rows [run_offsets[r], run_offsets[r + 1]) (int64 [R + 1], device).
 * Every entry of run_offsets is clamped into [0, Ttot] and a descending pair is an empty run; rank[r] is clamped into [0, k];
 * a run number of group_runs outside [0, R) is skipped: nothing read from memory is an address or a trip count unchecked.
 * All arithmetic is float64 (a float32 sum of y.y cannot resolve rss = 2e-5 y.y, the BOLD case), no float atomics, every order
 * fixed: outputs are bit-identical from call to call, and a (run, vertex) result does not depend on R, on M, on the other runs
 * of the call or on how the caller cuts the runs into calls (k of the call included: zero columns are never touched).
 *
 * glm_project: a[r][j][m] = sum_t Q[t][j] * y[t][m] (float64 [R][k][Mp]) and yy[r][m] = sum_t y[t][m]^2 (float64 [R][Mp]), each
 *   ONE chain acc = fma(q, y, acc) from 0 over ascending t of the run -- for a run of T >= chebgcn_glm_query(4) rows one chain
 *   per slice: n = min(chebgcn_glm_query(6), T / chebgcn_glm_query(5)) slices of ceil(T / n) consecutive rows (a function of T
 *   alone), the slices' sums added to the first one's in ascending order (plain float64 additions).  What the pad [M, Mp) of
 *   series holds (NaN included) never reaches a result; the pad of a and yy is written as zero.  k above chebgcn_glm_query(1) columns runs in panels of that many
 *   (the last one narrower), the scan re-read once per panel, yy formed in the first.  One pass otherwise.
 *   chebgcn_last_dispatch(): glm_project_kernel<NJ> per panel, NJ = its columns, joined by " + ".
 * glm_finish, per (run, vertex), T = the run's rows, dof = T - k_r:
 *     ssq = 0; ssq = fma(a_j, a_j, ssq), j ascending;   rss = yy - ssq, taken as 0 where rss < 4 (T + k_r) 2^-53 yy (the
 *     round-off of that subtraction; measured 5e-15 yy against this floor of 1.4e-13 yy at T = 284, k = 22);
 *     sigma2 = dof > 0 ? rss / dof : 0;   per contrast  e = 0; e = fma(u_j, a_j, e), j ascending;   variance = sigma2 * unorm2;
 *     t = variance > 0 ? e / sqrt(variance) : 0   (never NaN for finite input);   beta_p = fma chain of B[p][j] a_j likewise.
 *   eff64 / var64: float64 [R][C][Mp] (for glm_combine); effect / variance / t: float32 [R][C][Mp], each rounded ONCE from the
 *   float64 value; beta: float32 [R][P][Mp].  Each of the three sets may be NULL (B with beta), at least one is given.
 *   The pad [M, Mp) of every output plane of glm_finish and of glm_finish_ar1 (rho_out included) is scratch, as the conventions
 *   above say of every plane: it is written (with what the pads of the sums give) and nothing may be read from it; nothing
 *   outside the [R][.][Mp] planes is written.
 *   chebgcn_last_dispatch(): glm_finish_kernel.
 * glm_combine: fixed effects over the runs of a group.  group_ptr int32 [S + 1] / group_runs int32 [nruns] (device): group g is
 *   the runs group_runs[group_ptr[g] .. group_ptr[g + 1]), summed in that order (the caller lists them ascending), n of them:
 *     effect = (sum_r e_r) / n;   variance = (sum_r variance_r) / (n * n);   t = variance > 0 ? effect / sqrt(variance) : 0
 *   float64 from eff64 / var64, ONE rounding to float32; outputs [S][C][M] contiguous (no pad).
 *   chebgcn_last_dispatch(): glm_combine_kernel.
 * glm_query: 0 vertices of a project workgroup, 1 columns of a panel, 2 the largest k, 3 the largest C, 4 the run length from
 *   which the time loop is split, 5 the least rows of a slice, 6 slices at most, 7 the largest P, 8 runs of one call at most;
 *   -1 for anything else.
 * glm_workspace: bytes of a and yy together for R runs (yy follows a; 0: arguments out of range).
 * Limits: k <= 64, C <= 32, P <= 64, R <= 65535 per call, S <= 65535, Ttot * Mp <= 2^39: CHEBGCN_EUNSUPPORTED beyond, before
 * any launch, as every CHEBGCN_EINVAL (NULL, counts <= 0, pointers not aligned to their element; series to 8 bytes).  The calls neither synchronise nor allocate. */
int chebgcn_glm_query(int what);
size_t chebgcn_glm_workspace(int R, int M, int k);
int chebgcn_glm_project(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, const double* Q, int k, double* a,
                        double* yy, chebgcn_stream stream);
int chebgcn_glm_finish(const double* a, const double* yy, const int64_t* run_offsets, int64_t Ttot, const int32_t* rank, const double* U,
                       const double* unorm2, const double* B, int R, int M, int k, int C, int P, double* eff64, double* var64,
                       float* effect, float* variance, float* t, float* beta, chebgcn_stream stream);
int chebgcn_glm_combine(const double* eff64, const double* var64, const int32_t* group_ptr, const int32_t* group_runs, int nruns, int R,
                        int S, int C, int M, float* effect, float* variance, float* t, chebgcn_stream stream);

/* ---- first-level GLM with AR(1) prewhitening: generalised least squares per (run, vertex) (glm.first_level(noise='ar1')) ---------
 * Noise covariance sigma^2 rho^|i-j| / (1 - rho^2) inside a run: exact GLS for a stationary AR(1), the first row scaled
 * (Prais-Winsten), not dropped.  With K(rho) = (1 + rho^2) I - rho (Sh + Sh^T) - rho^2 (e_0 e_0^T + e_L e_L^T), Sh the one-row shift
 * inside the run and L = T - 1 its last row, the fit is the least-squares fit under y^T K y.  Besides the tables of the OLS
 * entries (Q, u, B, rank, run_offsets: as above, same clamps) the caller hands, per run,
 *   W = [Q | Qs]        float64 [Ttot][2k]: Qs = Sh Q + Sh^T Q, row t = Q[t - 1] + Q[t + 1] with zero beyond the ends of the run;
 *                       columns [k_r, k) and [k + k_r, 2k) are zero
 *   D = Q^T Qs          float64 [R][k][k], symmetric;   E = q_0 q_0^T + q_L q_L^T   float64 [R][k][k] (rows 0 and L of Q)
 * glm_project_ar1: ah[r][j][m] = sum_t W[t][j] y[t][m] (float64 [R][2k][Mp]: a = Q^T y, then h = Qs^T y), s0[r][m] = y.y and
 *   s1[r][m] = sum_{t > first row of the run} y[t][m] y[t - 1][m] (float64 [R][Mp] each): the fma chains, the slices (a function of
 *   T alone) and the panels of glm_project over the 2k columns; the s1 term of row t belongs to the slice of row t, the first row
 *   of a later slice pairs with the last row of the slice before it, the first row of a run with nothing (a lag never crosses
 *   a run boundary).  Pad columns as for glm_project.  chebgcn_last_dispatch(): glm_project_ar1_kernel<NJ> per panel, " + ".
 * glm_finish_ar1, per (run, vertex), T the run's rows, y_0 / y_L its first and last sample (read from series; pad columns and
 *   empty runs give 0), every sum an fma chain from 0 over ascending j < k_r unless stated:
 *     rho_given = 0:  ssq = a.a;  rss = s0 - ssq with the floor of glm_finish;  num = (s1 - a.h) + 0.5 * a.(D a), (D a)_i its own
 *       chain over j;  rho = num / rss clamped to +-0.99 (RHO_MAX), 0 where rss is 0.   rho_given = 1: rho as passed.
 *     c1 = fma(rho, rho, 1), r2 = rho * rho;   M_ij = fma(-r2, E_ij, fma(-rho, D_ij, i == j ? c1 : 0))
 *     g_i = fma(-r2, fma(q0_i, y_0, qL_i * y_L), fma(-rho, h_i, c1 * a_i));   yKy = fma(-r2, fma(y_0, y_0, y_L * y_L), fma(-2 rho, s1, c1 * s0))
 *     Cholesky M = L L^T by columns j ascending: x_ij = M_ij, x_ij = fma(-L_ip, L_jp, x_ij) over p < j ascending;
 *       L_jj = sqrt(x_jj), d_j = 1 / L_jj, L_ij = x_ij * d_j (a pivot not > 0 -- impossible for |rho| < 1 in exact arithmetic --
 *       gives L_jj = d_j = 0 and a zero column, never NaN)
 *     forward solves, columns j ascending: z_j = x_j * d_j, then x_i = fma(-L_ij, z_j, x_i) for i > j, from x = g; the same from
 *       x = u_c for w_c;   zz = z.z, ww_c = w_c.w_c, e_c = chain of fma(w_cj, z_j, e)
 *     rss* = yKy - zz, taken as 0 where rss* < 4 (T + k_r) 2^-53 (1 + |rho|)^4 / (1 - |rho|)^2 s0.  The floor: s0, s1, a, h carry
 *       relative round-off (T + k_r) 2^-53 of sums bounded by y.y, and enter yKy and g with weights of at most (1 + |rho|)^2;
 *       a backward-stable Cholesky solve is exact for M + dM, |dM| <= c k 2^-53 |M|, which moves g.M^-1 g by x^T dM x with
 *       x = M^-1 g, |M| <= (1 + |rho|)^2 and |x|^2 <= (1 + |rho|)^2 / (1 - |rho|)^2 y.y (the eigenvalues of K lie in
 *       [(1 - |rho|)^2, (1 + |rho|)^2]); the product of the two bounds dominates.  At rho = 0 it is the floor of glm_finish.
 *     sigma2 = dof > 0 ? rss* / dof : 0, dof = T - k_r (no correction for estimating rho);   variance_c = sigma2 * ww_c;
 *     t = variance > 0 ? e / sqrt(variance) : 0.   A vertex constant in time: rho = 0, variance = 0, t = 0, never NaN.
 *     beta (with B): back substitution L^T v = z over rows q DESCENDING (v_q = x_q * d_q, x_i = fma(-L_qi, v_q, x_i) for i < q),
 *       then beta_p = chain of fma(B[p][j], v_j, s).
 *   Outputs as for glm_finish, plus rho_out float32 [R][Mp] (the estimate, or the given value).  Every value is rounded ONCE to
 *   float32.  No chain depends on k of the call, on M, on the other runs or on the rank bucket: results are bit-identical under
 *   any batching.  A given rho outside (-1, 1) (NaN included): CHEBGCN_EINVAL.
 *   chebgcn_last_dispatch(): glm_finish_ar1_kernel<KB>, KB = chebgcn_glm_ar1_query(100 + k) the rank bucket (8, 16, 32 or 64).
 * glm_ar1_query: 0 waves of a finish workgroup, 1 contrasts per forward solve, 100 + k the rank bucket of k, 200 + k the vertices
 *   of a finish workgroup at that k (k in [1, 64]); -1 for anything else.
 * glm_ar1_workspace: bytes of ah, s0 and s1 together for R runs (s0 follows ah, s1 follows s0; 0: arguments out of range).
 * Limits, alignment and the order of the checks as for the OLS entries; series to 8 bytes for the projection, 4 for the finish.
 * The calls neither synchronise nor allocate. */
int chebgcn_glm_ar1_query(int what);
size_t chebgcn_glm_ar1_workspace(int R, int M, int k);
int chebgcn_glm_project_ar1(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, const double* W, int k,
                            double* ah, double* s0, double* s1, chebgcn_stream stream);
int chebgcn_glm_finish_ar1(const double* ah, const double* s0, const double* s1, const float* series, const double* W,
                           const int64_t* run_offsets, int64_t Ttot, const int32_t* rank, const double* D, const double* E,
                           const double* U, const double* B, int R, int M, int k, int C, int P, int rho_given, double rho,
                           double* eff64, double* var64, float* effect, float* variance, float* t, float* beta, float* rho_out,
                           chebgcn_stream stream);

/* ---- single-trial patterns: least squares - separate, one GLM per trial (glm.single_trial) --------------------------------------
 * Per run, trial j's model is [x_j | o_j1 .. o_jG | N]: its own regressor, the other trials summed per condition (G conditions;
 * or all of them in one column, G = 1), the nuisance columns N.  The caller factors N on the host (Qn orthonormal, rank q_r), forms
 * S = the G sums of the trial columns X and Z = (I - Qn Qn^T) [X | S], runs glm_project over the table [Qn | Z_S | 0] of k >= q_r + G
 * columns (so of run r the planes a[r][0 .. q_r) are an = Qn^T y and a[r][q_r .. q_r + G) are c = Z_S^T y), and hands glm_trials
 *   Z              float64 [Ttot][nmax]: row t belongs to the run that contains t; column j = z_j, zero beyond the run's trials
 *   trial_offsets  int64 [R + 1] (device): the trials of run r are the rows [trial_offsets[r], trial_offsets[r + 1]) of the flat
 *                  per-trial tables and of the outputs, at most nmax of them
 *   a, yy, k       what glm_project returned for these runs;   q_rank int32 [R] = q_r
 *   own  int32 [N]          the condition of trial i (0 when G = 1; -1: none of the sums holds the trial)
 *   rank int32 [N]          r_i = rank of H_i = D_i^T (I - Qn Qn^T) D_i, D_i = [x_i | S_g - [g = own_i] x_i], (1 + G)^2
 *   w    float64 [N][G1]    the first row of pinv(H_i), G1 = 1 + G
 *   F    float64 [N][G1][G1]   any factor with F^T F = pinv(H_i), rows at and beyond r_i zero
 * Per (trial i of run r, vertex), T the run's rows, p = z_i^T y formed like a column of glm_project (the same chains, slices
 * and panels of chebgcn_glm_trials_query(1) trial columns; the last panel has exactly its own), float64, every sum an fma chain
 * from 0 over ascending indices:
 *     d_0 = p, d_{1+g} = c_g - (g == own_i ? p : 0);   beta = sum_l w_l d_l;
 *     ssq = chain of an_j^2 over j < q_r CONTINUED by (F d)_j^2 over j < r_i, (F d)_j its own chain over l;
 *     rss = yy - ssq, taken as 0 where rss < 4 (T + q_r + r_i) 2^-53 yy (the floor of glm_finish);   dof = T - q_r - r_i;
 *     variance = (dof > 0 ? rss / dof : 0) * w_0;   t = variance > 0 ? beta / sqrt(variance) : 0.
 * beta / variance / t: float32 [N][Mp], each nullable (at least one given), each value rounded ONCE; pad columns are written as
 * zero whatever the pads of series, a and yy hold.  The trial projections are never stored: the epilogue runs in the workgroup
 * that formed them.  Clamps: run_offsets into [0, Ttot], trial_offsets into [0, N] (a run's count to nmax), q_rank into
 * [0, k - G], own into [-1, G), rank into [0, G1].  A (run, trial, vertex) result is the same bits whatever else the call holds,
 * whatever M, nmax and k are.  No float atomics; the call neither synchronises nor allocates.
 * chebgcn_last_dispatch(): glm_trials_kernel<NJ> per panel, NJ = its columns, joined by " + ".
 * glm_trials_query: 0 vertices of a workgroup, 1 trial columns of a panel, 2 the largest G1, 3 the largest k, 4 the largest nmax,
 *   5 runs of one call at most; -1 for anything else.
 * Limits: G1 <= 16, k <= 64, nmax <= 4096, R <= 65535, Ttot * Mp and N * Mp <= 2^39: CHEBGCN_EUNSUPPORTED beyond, before any
 * launch, as every CHEBGCN_EINVAL (NULL, counts <= 0, k < G, pointers not aligned to 8 bytes, the int32 tables to 4). */
int chebgcn_glm_trials_query(int what);
int chebgcn_glm_trials(const float* series, int64_t Ttot, const int64_t* run_offsets, int R, int M, const double* Z, int nmax,
                       const int64_t* trial_offsets, const double* a, const double* yy, int k, const int32_t* q_rank,
                       const int32_t* own, const int32_t* rank, const double* w, const double* F, int G1, int64_t N, float* beta,
                       float* variance, float* t, chebgcn_stream stream);

/* ---- searchlight decoding: cross-validated Gaussian naive Bayes at every centre (searchlight.searchlight) ------------------------
 * The caller sorts the S samples so that the test samples of one MODEL (a training set: a (group, fold) pair, or a fold) are
 * contiguous, and hands the kernels (all device memory)
 *   Xt         float32 [M][Sp], Sp = chebgcn_plane_stride(S): the patterns vertex-major, sample s of vertex v at Xt[v * Sp + s].
 *              What the pad columns [S, Sp) hold (NaN included) never reaches a result.
 *   test_ptr   int32 [NM + 1]: the test samples of model m are the columns [test_ptr[m], test_ptr[m + 1])
 *   lists      int32 pointer / index pairs of sample numbers: list_ptr [NM + 1] the whole training set of every model (spread),
 *              class_ptr [NM * C + 1] the training samples of every (model, class), model-major (fit)
 *   rowptr / colidx   int32 CSR [U + 1] / [nnz]: row u lists the vertices centre u sees, in the caller's vertex order
 *   sgroup / slabel / sorig   int32 [S]: of sample s its group in [0, G), its class in [0, C), its number in the caller's order
 * Every pointer-table entry is clamped into its array and a descending pair is an empty list; a sample number outside [0, S), a
 * vertex outside [0, M), a group outside [0, G) is skipped: nothing read from memory is an address or a trip count unchecked.
 * All arithmetic is float64 in the centred form (BOLD has mean / sd of 1e2 .. 1e4: the expanded quadratic cancels by its
 * square), no float atomics, every order fixed: outputs are bit-identical from call to call and do not depend on how the caller
 * cuts the centres into calls (u0, Ub) or on the other models of the call.
 *
 * Moments of a list at a vertex, x_i = Xt[v][list[i]], i ascending over the n entries inside [0, S):
 *     s = 0; s = s + x_i;   mu = s / n;   ss = 0; d = x_i - mu, ss = fma(d, d, ss);   variance = ss / n     (n = 0: all 0)
 * searchlight_spread: spread[m][v] (float64 [NM][M]) = the variance of list m at v.  The caller takes
 *   eps[m] = var_smoothing * max_v spread[m][v] (any reduction: a maximum has no order).
 *   chebgcn_last_dispatch(): searchlight_spread_kernel.
 * searchlight_fit, per (model, vertex), NC = chebgcn_searchlight_query(100 + C) the class bucket (2, 4, 8, 16 or 32):
 *     per class c < C the moments of list m * C + c;   pooled: variance_c = (sum_c ss_c, c ascending) / (sum_c n_c) for every c;
 *     var = variance_c + eps[m];   h = 1 / (2 var);   lg = 0.5 * log(2 pi var);   h = lg = 0 where var is not > 0 (such a
 *     vertex contributes nothing), and mu = h = lg = 0 for a class without samples and for the classes [C, NC).
 *   par: float64 [NM][M][NC][2] = (mu, h);  lg: float64 [NM][M][NC] -- contiguous per (model, vertex), which is what a score
 *   wave reads per neighbour.  chebgcn_last_dispatch(): searchlight_fit_kernel.
 * searchlight_score, for the centres [u0, u0 + Ub) of the U rows:
 *     base[m][ub][c] = logprior[m][c] - L,   L = 0; L = L + lg[m][v][c] over the entries v of row u0 + ub in ascending entry order
 *       (float64 [NM][Ub][NC]: the caller's workspace; logprior float64 [NM][NC]);
 *     per test sample s of model m:   a_c = 0;  t = (double)Xt[v][s] - mu,  a_c = fma(t * h, t, a_c)  over the same entries in the
 *       same order;   score_c = base_c - a_c;   prediction = the first c < C with the largest score;
 *     correct[sgroup[s]][slabel[s]][u] += 1 (int32 atomics: any order is the same result) where the prediction is slabel[s].
 *   correct: int32 [G][C][U], which the call ADDS to (the caller zeroes it); scores: float64 [S][C][U] or NULL, predictions:
 *   uint8 [S][U] or NULL, both indexed by sorig[s].  tmax: the most test samples of a model, 1 <= tmax <= S -- it sizes the
 *   launch; samples of a model beyond its first tmax are not scored.
 *   chebgcn_last_dispatch(): searchlight_base_kernel + searchlight_score_kernel<NC>.
 * searchlight_query: 0 lanes of a score wave, 1 centres of a score workgroup, 2 neighbours in flight (class buckets above query
 *   8), 3 the largest C, 4 vertices of a spread / fit workgroup, 5 models of one call at most, 6 tiles of a model at most,
 *   7 groups at most, 8 the widest NARROW class bucket, 9 test samples of a lane in a narrow bucket (one in the others: a
 *   workgroup covers query 0 times this many consecutive test samples of a model), 10 neighbours in flight in a narrow bucket,
 *   100 + C the class bucket of C classes (1 <= C <= 32); -1 for anything else.  None of these reaches a result.
 * Limits: 2 <= C <= 32, NM <= 65535, G <= 2^20, tmax <= 65535 * 64, Ub <= (2^31 - 1) / 32: CHEBGCN_EUNSUPPORTED beyond, before any
 * launch, as every CHEBGCN_EINVAL (NULL, counts <= 0, centres outside [0, U), pointers not aligned to their element).  The calls
 * neither synchronise nor allocate. */
int chebgcn_searchlight_query(int what);
int chebgcn_searchlight_spread(const float* Xt, int S, int M, const int32_t* list_ptr, const int32_t* list_idx, int nidx, int NM,
                               double* spread, chebgcn_stream stream);
int chebgcn_searchlight_fit(const float* Xt, int S, int M, const int32_t* class_ptr, const int32_t* class_idx, int nidx, int NM, int C,
                            int pooled, const double* eps, double* par, double* lg, chebgcn_stream stream);
int chebgcn_searchlight_score(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U, int u0, int Ub,
                              const int32_t* test_ptr, int tmax, int NM, int C, const double* par, const double* lg,
                              const double* logprior, const int32_t* sgroup, const int32_t* slabel, const int32_t* sorig, int G,
                              double* base, int32_t* correct, double* scores, uint8_t* predictions, chebgcn_stream stream);

/* ---- searchlight decoding with shrinkage LDA: a covariance, its Cholesky factor and its discriminants per (model, centre) --------
 * (searchlight.searchlight(classifier='lda')).  The tables are those of the naive-Bayes calls above; par is what
 * chebgcn_searchlight_fit wrote with eps = 0 (only the means par[m][v][c][0] are read), logprior float64 [NM][NC],
 * NC = chebgcn_searchlight_query(100 + C).  centres: int32 [Ub] row numbers of this launch (one workgroup per (centre, model));
 * bucket: 32, 64 or 128 -- a row longer than the bucket (or empty) is skipped and nothing of it is written.
 * The model, for model m and a row of vertices v_0 < ... < v_{P-1}, P <= 128, all in float64:
 *     n_c = entries of list m * C + c inside [0, S),  n = sum n_c;   mu_cv = par[m][v][c][0];
 *     m_v = (a = 0; a = fma(n_c, mu_cv, a), c ascending) / n;   d_cv = mu_cv - m_v;
 *     r_kv = (double)Xt[v][k] - mu_{c v} for the entries k of the class lists, class 0's list first, each in list order;
 *     S_ij = (a = 0; a = fma(r_ki, r_kj, a), one chain over those samples in that order) / n;
 *     tr = sum_i S_ii (i ascending),  nu = tr / P;
 *     g = shrinkage, or if shrinkage < 0 the Ledoit-Wolf coefficient of the residuals:
 *         q_k = (sum of r_ki^2 over even i ascending) + (the same over odd i),  beta_ = fma(q_k, q_k, .) in sample order,
 *         delta_ = per i ascending fma(S_ii, S_ii, .) then fma(2, sum_{j < i} S_ij^2, .),
 *         beta = (beta_ / n - delta_) / (P n),  delta = (delta_ - 2 nu tr + P nu^2) / P,  beta = min(beta, delta),
 *         g = beta / delta (0 where beta == 0), clipped into [CHEBGCN_LDA_SHRINK_MIN, 1];
 *     Sigma = (1 - g) S + g nu I;   Sigma = L L^T: element (i, j) receives fma(-L_ik, L_jk, .) for k ascending, then the
 *         square root (i = j) or the division by L_jj -- no pivoting: the floor on g bounds the condition number by about P / g;
 *     L y_c = d_c (k ascending), L^T w_c = y_c (k descending), each element's chain followed by the division by L_ii;
 *     b_c = logprior[m][c] - 0.5 (a = 0; a = fma(d_cv, w_cv, a), v ascending);
 *     score[s][c][u] = b_c + (a = 0; a = fma(w_cv, (double)Xt[v][s] - m_v, a), v ascending);  prediction = the first maximal class;
 *     correct[sgroup[s]][slabel[s]][u] += 1 where the prediction is slabel[s] (int32 atomics).
 *   Degenerate -- tr not > 0 (every vertex constant within every class), n = 0, or a pivot not > 0 and finite: w = 0 and
 *   b_c = logprior[m][c]; the prior decides and nothing is NaN.  The covariance does not depend on logprior.
 *   correct int32 [G][C][U] is ADDED to; scores float64 [S][C][U] / predictions uint8 [S][U] / gamma_out float64 [NM][U] (the g
 *   used) or NULL.  tmax as in searchlight_score.  Guards as above; a vertex outside [0, M) is a column of zeros (its w is 0), a
 *   centre outside [0, U) is skipped.  Every value is a function of (model, centre, lists) alone: bit-identical under any
 *   cut of the centres into launches, any order of centres, any other rows or models in the launch.  No float atomics.
 *   chebgcn_last_dispatch(): searchlight_lda_kernel<bucket>.
 * searchlight_lda_query: 0 threads of a workgroup, 1 the longest row (128), 2 training samples of a residual tile, 3 the largest
 *   C, 4 blocks along a side of the covariance triangle, 5 models at most, 6 tiles of a model at most, 7 groups at most, 8 the
 *   class count up to which the class tables in LDS are narrow, 100 + P the bucket of a row of P vertices (1 <= P <= 128); -1
 *   for anything else.
 * Limits: 2 <= C <= 32, NM <= 65535, G <= 2^20, tmax <= 65535 * 64, bucket in {32, 64, 128}: CHEBGCN_EUNSUPPORTED beyond, before
 * any launch, as every CHEBGCN_EINVAL (NULL, counts <= 0, a shrinkage that is neither negative nor in [1e-6, 1], pointers not
 * aligned to their element).  The call neither synchronises nor allocates. */
#define CHEBGCN_LDA_SHRINK_MIN 1e-6
int chebgcn_searchlight_lda_query(int what);
int chebgcn_searchlight_lda(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U,
                            const int32_t* centres, int Ub, int bucket, const int32_t* class_ptr, const int32_t* class_idx, int nidx,
                            const int32_t* test_ptr, int tmax, int NM, int C, const double* par, const double* logprior,
                            double shrinkage, const int32_t* sgroup, const int32_t* slabel, const int32_t* sorig, int G,
                            int32_t* correct, double* scores, uint8_t* predictions, double* gamma_out, chebgcn_stream stream);

/* ---- RSA searchlight: the cross-validated Mahalanobis ("crossnobis") distance of every pair of classes per (group, centre) ------
 * (searchlight.crossnobis).  A cell is a (group, partition); the NM cells are numbered group by group, cell_ptr int32 [G + 1]
 * gives the contiguous cells of every group (device memory, clamped into [0, NM]; a group of fewer than 2 cells is skipped and
 * nothing of it is written), class_ptr int32 [NM * C + 1] / class_idx int32 [nidx] list the samples of every (cell, class), and
 * par is what chebgcn_searchlight_fit wrote for these lists with one "model" per cell and eps = 0 (only the means
 * par[k][v][c][0] are read).  centres, bucket, Xt, rowptr, colidx as chebgcn_searchlight_lda.
 * The quantity, for group g with cells k0 <= k < k1, F = k1 - k0, and a row of vertices v_0 < ... < v_{P-1}, P <= 128, in float64:
 *     n_kc = entries of list k * C + c inside [0, S),  n = sum n_kc;   mu_kcv = par[k][v][c][0];
 *     m_v = (a = 0; a = fma(n_kc, mu_kcv, a), k ascending, c ascending inside) / n;   d_kcv = mu_kcv - m_v;
 *     r_sv = (double)Xt[v][s] - mu_{k c v} for the entries s of the lists, cell k0's class 0 first, c ascending inside a cell, each
 *         list in list order: the residuals about the CELL means;
 *     S_ij = (a = 0; a = fma(r_si, r_sj, a), one chain over those samples in that order) / n;
 *     tr, nu, the shrinkage g (given, or Ledoit-Wolf's of these residuals where shrinkage < 0), Sigma = (1 - g) S + g nu I and
 *         its Cholesky factor L: exactly as chebgcn_searchlight_lda states them (csrc/searchlight_ball.h holds both kernels' stages);
 *     u_kc = L^-1 d_kc:  element i receives fma(-L_ij, u_j, .) for j ascending, then the division by L_ii;
 *     T_cv = sum_k u_kcv, k ascending;
 *     for classes a < b:  q_ab = (x = 0; x = fma(u_kav - u_kbv, u_kav - u_kbv, x), k outer ascending, v ascending inside),
 *         t_ab = (x = 0; x = fma(T_av - T_bv, T_av - T_bv, x), v ascending),
 *         rdm[g][pair][u] = (t_ab - q_ab) / (F (F - 1) P)
 *     -- the mean over ordered pairs of different cells k != l of (u_ka - u_kb) . (u_la - u_lb) / P.  Pairs are numbered row-major
 *     over a < b (scipy.spatial.distance.squareform's order), C (C - 1) / 2 of them.
 *   Degenerate -- tr not > 0, n = 0, or a pivot not > 0 and finite: every distance of that (group, centre) is 0 and
 *   gamma_out[g][u] = -1; nothing is NaN.  Otherwise gamma_out float64 [G][U] (or NULL) receives the g used.
 *   rdm float64 [G][C (C - 1) / 2][U].  Guards as chebgcn_searchlight_lda: every pointer range is clamped, a centre outside [0, U)
 *   is skipped, sample numbers outside [0, S) are rows of zeros and are not counted, a vertex outside [0, M) is a column of
 *   zeros, a row longer than the bucket (or empty) is skipped with its outputs untouched.  Every value is a function of (group,
 *   centre, lists) alone: bit-identical under any cut of the centres into launches, any order of centres, any other rows or
 *   groups in the launch.  No float atomics.  chebgcn_last_dispatch(): searchlight_rdm_kernel<bucket>.
 * searchlight_rdm_query: 0 threads of a workgroup, 1 the longest row (128), 2 samples of a residual tile, 3 the largest C, 4 the
 *   most pairs of classes (496; a thread owns two beyond query 0), 5 cells at most (the models of chebgcn_searchlight_lda), 6 the
 *   class count up to which the class tables in LDS are narrow, 100 + P the bucket of a row of P vertices; -1 for anything else.
 * Limits: 2 <= C <= 32, NM <= 65535, bucket in {32, 64, 128}: CHEBGCN_EUNSUPPORTED beyond, before any launch, as every
 * CHEBGCN_EINVAL (NULL, counts <= 0, a shrinkage that is neither negative nor in [1e-6, 1], pointers not aligned to their
 * element, NM < 2 G: some group would hold fewer than 2 cells -- cell_ptr itself lives on the device and is guarded there).
 * The call neither synchronises nor allocates. */
int chebgcn_searchlight_rdm_query(int what);
int chebgcn_searchlight_rdm(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U,
                            const int32_t* centres, int Ub, int bucket, const int32_t* cell_ptr, const int32_t* class_ptr,
                            const int32_t* class_idx, int nidx, int NM, int C, const double* par, double shrinkage, int G,
                            double* rdm, double* gamma_out, chebgcn_stream stream);

/* ---- searchlight decoding with a linear SVM: one dual problem per class on the Gram matrix of every (model, centre) ---------------
 * (searchlight.searchlight(classifier='svc')).  Xt, rowptr, colidx, centres, test_ptr, sgroup, slabel, sorig, correct, scores,
 * predictions as chebgcn_searchlight_lda; list_ptr int32 [NM + 1] / list_idx int32 [nidx] are the training samples of every model
 * (the lists of chebgcn_searchlight_spread), whose labels are slabel[list_idx[.]]; models: int32 [NMb] model numbers of this launch
 * (one workgroup per (centre, model)); bucket: 32, 64 or 128 -- a model whose list is longer than the bucket (or empty) is skipped
 * and nothing of it is written.  Rows of ANY length are served: the state on chip depends on the training set alone.
 * The model, for model m with training samples k_0 < ... < k_{n-1} (list order), n <= 128, and a row of vertices
 * v_0 < ... < v_{P-1}, P >= 1.  Float64 throughout, EVERY OPERATION A SEPARATE CORRECTLY ROUNDED MULTIPLY, ADD OR DIVIDE: nothing is
 * fused (the file is compiled with contraction off), so a restatement in NumPy agrees bit for bit:
 *     m_v = ((double)Xt[v][k_0] + (double)Xt[v][k_1] + ...) / n:  one chain in list order, then one division (formed by this
 *         kernel; chebgcn_searchlight_fit's means are compiled with contraction on and are not used);
 *     x_iv = (double)Xt[v][k_i] - m_v, and the same for a test sample s;
 *     K_ij = (a = 0; a = a + x_iv x_jv, v ascending) for the training pairs (i >= j, symmetric) and every (test sample, training
 *         sample) pair; a vertex outside [0, M) contributes nothing;
 *     one-vs-rest with liblinear's regularised bias (fit_intercept=True, intercept_scaling=1: the kernel is K + 1).  Class c:
 *         t_i = +1 if slabel[k_i] == c, else -1;  q_ij = K_ij + 1;  Q_ij = t_i t_j q_ij;
 *         loss 0 (squared hinge): D = 1 / (2 C), no upper bound (Ub = +inf);   loss 1 (hinge): D = 0, Ub = C;
 *         Qd_i = q_ii + D  (>= 1: no division needs a guard, there is no degenerate branch);
 *     dual coordinate descent (Hsieh et al. 2008) in fixed cyclic order, no shuffling, no shrinking of the active set:
 *         alpha = 0, g_i = -1;  sweeps e = 1 .. max_iter, each visiting i = 0 .. n - 1:
 *             G = g_i;  PG = min(G, 0) if alpha_i == 0, max(G, 0) if alpha_i == Ub, else G;
 *             if PG != 0:  a = min(max(alpha_i - G / Qd_i, 0), Ub);  delta = a - alpha_i;  alpha_i = a;
 *                 for every j:  g_j = g_j + (t_i t_j) (delta q_ji);   at j = i additionally, as a second addition, g_i = g_i + delta D;
 *         after a sweep: stop if the sweep's max |PG| <= tol;
 *     score[s][c][u] = (a = 0; a = a + (alpha_j t_j) (K_sj + 1), j in list order);  prediction = the first maximal class;
 *     correct[sgroup[s]][slabel[s]][u] += 1 where the prediction is slabel[s] (int32 atomics).
 *   Two classes: the two problems are mirror images (the same Q, the same alpha), f_1 = -f_0 exactly; class 0 is solved and negated.
 *   At convergence this is scikit-learn's LinearSVC(loss=, C=, dual=True, fit_intercept=True, intercept_scaling=1, multi_class='ovr')
 *   on the row's columns centred by the training means.
 *   sweeps int32 [NM][U] (or NULL): the most sweeps any class of that (model, centre) ran;  residual float64 [NM][U] (or NULL): the
 *   largest last-sweep max |PG| over the classes.  correct is ADDED to.  Guards: every pointer range is clamped, a centre outside
 *   [0, U) or a model outside [0, NM) is skipped, a sample number outside [0, S) is a row of zeros of the centred patterns and is
 *   not counted in n, group and label numbers outside their ranges add nothing.  Every value is a function of (model, centre,
 *   lists) alone: bit-identical under any cut of the centres or models into launches and any order of them.  No float atomics.
 *   chebgcn_last_dispatch(): searchlight_svm_kernel<bucket>.
 * searchlight_svm_query: 0 threads of a workgroup, 1 the largest training set (128), 2 vertices of a tile, 3 the largest C, 4 test
 *   samples of a chunk, 5 models at most, 6 tiles of a model's test samples at most, 7 groups at most, 8 the largest max_iter,
 *   9 vertices of a super-tile (the means of so many vertices are formed at once), 100 + n the bucket of a training set of n
 *   samples (1 <= n <= 128); -1 for anything else.
 * Limits: 2 <= C <= 32 classes, NM and NMb <= 65535, G <= 2^20, tmax <= 65535 * 64, bucket in {32, 64, 128}: CHEBGCN_EUNSUPPORTED
 * beyond, before any launch, as every CHEBGCN_EINVAL (NULL, counts <= 0, C or tol not finite, C <= 0, tol < 0, a loss other than
 * 0 or 1, max_iter outside [1, 100000], pointers not aligned to their element).  The call neither synchronises nor allocates. */
int chebgcn_searchlight_svm_query(int what);
int chebgcn_searchlight_svm(const float* Xt, int S, int M, const int32_t* rowptr, const int32_t* colidx, int nnz, int U,
                            const int32_t* centres, int Ub, const int32_t* models, int NMb, int bucket, const int32_t* list_ptr,
                            const int32_t* list_idx, int nidx, const int32_t* test_ptr, int tmax, int NM, int C, double Creg, int loss,
                            double tol, int max_iter, const int32_t* sgroup, const int32_t* slabel, const int32_t* sorig, int G,
                            int32_t* correct, double* scores, uint8_t* predictions, int32_t* sweeps, double* residual,
                            chebgcn_stream stream);

/* ---- vertex order for the ordered recurrence kernels (host only) ----
 * The reference leaves the numbering of a graph's vertices to its caller (the coarsening's tree order, coarsening.py:168-215);
 * the network is invariant under a relabelling as long as everything per-vertex follows (cgcnn.vertex_order).  A graph whose
 * rows come sorted by descending length (graph.length_order) runs the ordered kernels; chebgcn_bank_order refines such an
 * order INSIDE its classes of equal row length so that the LDS reads of the gather spread over the banks (csrc/graph.hip).
 *   rowptr / colidx: CSR structure of the rescaled Laplacian in the length-sorted numbering (host memory);
 *   sweeps: passes of the pairwise-swap descent (0 = identity); perm_out[new label] = old label, M entries;
 *   stats (optional, 3 values): sum over the gather's lane sets of the fullest bank group before / after, swaps made.
 * Returns the identity where no ordered kernel serves the graph (nothing to gain).  Deterministic. */
int chebgcn_bank_order(int M, const int32_t* rowptr, const int32_t* colidx, int sweeps, int32_t* perm_out, int64_t* stats);

/* ---- functional connectivity matrices per run: shrunk covariance, correlation, precision, partial correlation (connectome) ------
 * series: [Ttot][Rp] float32 planes, Rp = chebgcn_plane_stride(R), run s = rows [run_offsets[s], run_offsets[s + 1]) (each offset
 * clamped into [0, Ttot], a descending pair an empty run), R regions.  The pad columns [R, Rp) may hold anything, NaN included:
 * what they hold never reaches a result.  workspace: chebgcn_connectome_workspace(S, R) bytes, 16-byte aligned: per run the
 * float64 matrix [Rp][Rp] and four vectors of Rp; connectome_cov fills it, connectome_finish consumes (and overwrites) it.
 * Everything is float64 until the one rounding to float32; no float atomics; every sum below has ONE order, a function of the
 * run's own T and of R alone, so a run's results are the same bits alone or among others, in any batch, in any call.
 * connectome_cov, per run, T its rows, x_ti the float32 sample of region i:
 *     mean_i = (sum_t (double)x_ti) / T                  one chain acc = acc + x over ascending t
 *     d_ti = (double)x_ti - mean_i
 *     q_t = sum_i d_ti^2                                 lane l: the chain fma(d, d, q) over i = l, l + 64, ...; then the 64 lanes by
 *                                                        the butterfly q = q + q(lane ^ s), s = 1, 2, .., 32
 *     beta_ = sum_t q_t^2                                class w = (t - t0) mod chebgcn_connectome_query(7): the chain fma(q, q, b)
 *                                                        over its rows ascending; then the classes added in ascending w
 *     C_ij = (sum_t d_ti d_tj) / T                       ONE chain fma(d_ti, d_tj, acc) from 0 over ascending t: a run is never
 *                                                        cut along time; C_ij and C_ji are the same bits
 *   chebgcn_last_dispatch(): connectome_centre_kernel + connectome_rowsq_kernel + connectome_cov_kernel.
 * connectome_finish, per run (kind: CHEBGCN_CONNECTOME_*; shrinkage: a number in [0, 1], or negative for Ledoit-Wolf):
 *     delta_ = sum_ij C_ij^2                             thread u of chebgcn_connectome_query(6): the chain fma(c, c, acc) over the
 *                                                        entries e = i R + j = u, u + 512, ...; then the tree red[u] += red[u + h],
 *                                                        h = 256, 128, .., 1.  tr = sum_i C_ii by the same tree
 *     mu = tr / R;  beta = (beta_ / T - delta_) / (R T);  delta = ((delta_ - (2 mu) tr) + (R mu) mu) / R, every operation
 *     rounded on its own (no fused multiply-add: for one region the terms then cancel to exactly 0)
 *     s = max(min(beta, delta), 0) / delta, and 0 where delta is not > 0  (never a negative zero)
 *     Sigma_ij = fma(1 - s, C_ij, i == j ? s mu : 0)
 *     covariance: Sigma.   correlation: Sigma_ij / sqrt(Sigma_ii Sigma_jj), 0 where that product is not > 0; the diagonal 1.
 *     precision P = Sigma^-1 by Cholesky without pivoting, Sigma = L L^T:
 *         L_ij = (Sigma_ij - sum_{p < j} L_ip L_jp) (1 / L_jj), the chain fma(-L_ip, L_jp, acc) over ascending p, L_jj = sqrt(pivot);
 *         M = L^-1:  M_ic = (delta_ic - sum_{c <= p < i} L_ip M_pc) (1 / L_ii), the chain fma(-L_ip, M_pc, acc) over ascending p;
 *         P_ij = sum_{p >= max(i, j)} M_pi M_pj, the chain fma(M_pi, M_pj, acc) over ascending p, formed for i >= j and mirrored.
 *       A pivot that is not > 4 R 2^-53 Sigma_jj (the round-off of its own chain), or not finite, makes the run DEGENERATE: its
 *       flag is 1 and its matrix the identity (precision and partial correlation alike); no NaN for finite input.
 *     partial correlation: -P_ij / sqrt(P_ii P_jj), the diagonal 1.
 *   matrices: float32 [S][R][R], each value rounded ONCE, each matrix symmetric bit for bit.  shrinkage_out float64 [S],
 *   degenerate int32 [S] (always 0 for covariance and correlation).
 *   chebgcn_last_dispatch(): connectome_finish_kernel<plain> (covariance, correlation), or connectome_finish_kernel<inverse> +
 *   connectome_invert_kernel + connectome_gram_kernel.
 * connectome_mean: mean[i][j] = (float)((sum over the runs s with degenerate[s] == 0, ascending s, of (double)matrices[s][i][j]) /
 *   their number), zeros where there is none.  float32 [R][R].  chebgcn_last_dispatch(): connectome_mean_kernel.
 * connectome_query: 0 the largest R, 1 runs of one call, 2 side of a covariance / gram tile, 3 rows of a tile's operands in LDS at
 *   once, 4 columns of a Cholesky panel, 5 finished columns staged in LDS at once, 6 threads of a finish workgroup, 7 row classes
 *   of beta_; -1 otherwise.
 * connectome_workspace: bytes for S runs of R regions (0: arguments out of range).
 * Limits: R <= 512, S <= 65535 per call (connectome_mean: S <= 2^24), Ttot * Rp <= 2^39: CHEBGCN_EUNSUPPORTED beyond, before any
 * launch, as every CHEBGCN_EINVAL (NULL, counts <= 0, an unknown kind, a shrinkage above 1 or NaN, a workspace too small, series
 * and workspace not aligned to 16 bytes, the other pointers to their element).  The calls neither synchronise nor allocate. */
enum {
    CHEBGCN_CONNECTOME_COVARIANCE = 0,
    CHEBGCN_CONNECTOME_CORRELATION = 1,
    CHEBGCN_CONNECTOME_PRECISION = 2,
    CHEBGCN_CONNECTOME_PARTIAL = 3
};
int chebgcn_connectome_query(int what);
size_t chebgcn_connectome_workspace(int S, int R);
int chebgcn_connectome_cov(const float* series, int64_t Ttot, const int64_t* run_offsets, int S, int R, double* workspace,
                           size_t workspace_bytes, chebgcn_stream stream);
int chebgcn_connectome_finish(double* workspace, size_t workspace_bytes, const int64_t* run_offsets, int64_t Ttot, int S, int R, int kind,
                              double shrinkage, float* matrices, double* shrinkage_out, int32_t* degenerate, chebgcn_stream stream);
int chebgcn_connectome_mean(const float* matrices, const int32_t* degenerate, int S, int R, float* mean, chebgcn_stream stream);

/* ---- tangent-space connectivity: a batched symmetric eigensolver and the products around it (connectome.tangent) ----------------
 * All matrices are float64 [S][R][R], dense (row stride R), 8-byte aligned; flags and counters int32.  No float atomics; every sum
 * below has ONE order, a function of R alone, so a matrix's results are the same bits alone or among others, in any call.
 * connectome_sigma: Sigma of connectome_finish (the same body: delta_, mu, the shrinkage, Sigma_ij = fma(1 - s, C_ij, ...)) from the
 *   workspace connectome_cov left (overwritten), kept in float64: sigma [S][R][R], shrinkage_out [S].  (float)sigma is the
 *   covariance kind of connectome_finish bit for bit.  chebgcn_last_dispatch(): connectome_sigma_kernel.
 * sym_eigh: A_s = V_s diag(w_s) V_s^T for symmetric A_s (the lower and the upper triangle are both read; they must agree).
 *   w [S][R] in NO particular order, Vt [S][R][R] with ROW p the eigenvector of w[p] (V transposed), sweeps [S], converged [S].
 *   A block Jacobi method on X = A V and V (X <- A, V <- I), columns in blocks of chebgcn_tangent_query(2) = 8, the block pairs of
 *   a sweep in round-robin order (player nb - 1 or the bye of an odd count stays, the others turn), one launch per step, a
 *   workgroup per (pair, matrix); a matrix of one block works on that block alone.  Per pair, with x_i, v_i its 16 columns:
 *       T_ij = ((sum_r v_ir x_jr) + (sum_r v_jr x_ir)) / 2     each sum ONE chain fma(v, x, acc) over ascending rows r; T_ij and T_ji
 *                                                               come from the same two chains: T = sym(V^T A V) on the pair
 *       a two-sided Jacobi on T accumulating Q, pairs (p, q) in the round-robin order of 16 players, up to query(7) sweeps:
 *       zeta = (T_qq - T_pp) / (2 T_pq), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (sign(0) = 1), c = 1 / sqrt(1 + t^2), s = c t;
 *       a pair is left alone when |T_pq| <= max(R 2^-53 sqrt(|T_pp T_qq|), R 2^-53 max_ij |A_ij|), or is not finite
 *       X_blk <- X_blk Q, V_blk <- V_blk Q                     each entry ONE chain over the pair's columns in ascending order
 *   T is formed from V^T X and not from X^T X: the Gram matrix X^T X = V^T A^2 V cannot tell the eigenvalues lambda and -lambda
 *   apart (A = [[0, 1], [1, 0]] has orthogonal columns and no rotation ever starts), and the mean of tangent vectors is indefinite.
 *   A sweep in which no workgroup rotated ends the matrix (rotations are counted with integer atomics); finished matrices skip
 *   later steps; after query(4) = 40 sweeps a matrix still rotating is reported with converged = 0.  sweeps counts the last,
 *   idle sweep too.  w_p = sum_r v_pr x_pr, the Rayleigh quotient, signed, one chain over ascending r.
 *   The call reads ONE int32 back per sweep (the number of matrices still open) and synchronises the stream for it: the only
 *   entry of this family that does.  workspace: chebgcn_tangent_workspace(S, R) bytes, 8-byte aligned.
 *   chebgcn_last_dispatch(): tangent_eigh_init_kernel + tangent_eigh_step_kernel + tangent_eigh_sweep_kernel +
 *   tangent_eigh_values_kernel.
 * sym_function: out_s = V_s diag(f(a w_s)) V_s^T, f one of CHEBGCN_SYM_*: out_ij = sum_p (f_p Vt_pi) Vt_pj, ONE chain fma over
 *   ascending p, formed for i >= j and mirrored.  out is float64, or float32 rounded once (out_float32 = 1).  A value a w_p that is
 *   not finite, that log, sqrt or 1/sqrt cannot take (not > 0), or whose exp overflows sets flags[s] = 1; a matrix whose flag is
 *   set (by this call or before it) comes out as zeros.  flags are never cleared here.  fvals: scratch of S R doubles.
 *   chebgcn_last_dispatch(): tangent_fvals_kernel + tangent_product_kernel<lower>.
 * sym_congruence: out_s = W A_s W for ONE symmetric W [R][R] and symmetric A_s: scratch_s = A_s W (scratch_ij = sum_p A_pi W_pj),
 *   then out_ij = sum_p W_pi scratch_pj for i >= j, mirrored; each ONE chain fma over ascending p.  scratch: S R R doubles.
 *   chebgcn_last_dispatch(): tangent_product_kernel<full> + tangent_product_kernel<lower>.
 * sym_mean: acc_ij = (first ? 0 : acc_ij) + sum over the s with flags[s] == 0, ascending, of matrices[s][i][j], the chain
 *   acc = acc + m: runs may come in any number of calls.  With n_total > 0 the call also writes mean = acc / n_total and
 *   norm[0] = sqrt(sum_ij mean_ij^2): thread u of 512 the chain fma(m, m, acc) over e = i R + j = u, u + 512, ..., then the tree
 *   red[u] += red[u + h], h = 256, 128, .., 1.  chebgcn_last_dispatch(): tangent_mean_kernel (+ tangent_norm_kernel).
 * tangent_query: 0 the largest R, 1 matrices of one call, 2 columns of a Jacobi block, 3 threads of a step workgroup (a thread's
 *   second row), 4 the cap of sweeps, 5 side of a product tile, 6 rows of a tile's operands in LDS at once, 7 sweeps of the
 *   Jacobi inside a pair; -1 otherwise.  tangent_workspace: bytes of sym_eigh's workspace (0: arguments out of range).
 * Limits: R <= 512, S <= 65535 per call (sym_mean: S <= 2^24): CHEBGCN_EUNSUPPORTED beyond, before any launch, as every
 * CHEBGCN_EINVAL (NULL, counts <= 0, an unknown function, a = NaN or inf, a workspace too small, a pointer not aligned to its
 * element, scratch or Vt aliasing an operand).  Except for sym_eigh's readback the calls neither synchronise nor allocate. */
enum {
    CHEBGCN_SYM_LOG = 0,
    CHEBGCN_SYM_EXP = 1,
    CHEBGCN_SYM_SQRT = 2,
    CHEBGCN_SYM_RSQRT = 3
};
int chebgcn_connectome_sigma(double* workspace, size_t workspace_bytes, const int64_t* run_offsets, int64_t Ttot, int S, int R,
                             double shrinkage, double* sigma, double* shrinkage_out, chebgcn_stream stream);
int chebgcn_tangent_query(int what);
size_t chebgcn_tangent_workspace(int S, int R);
int chebgcn_sym_eigh(const double* A, int S, int R, double* w, double* Vt, int32_t* sweeps, int32_t* converged, void* workspace,
                     size_t workspace_bytes, chebgcn_stream stream);
int chebgcn_sym_function(const double* w, const double* Vt, int S, int R, int func, double a, void* out, int out_float32, int32_t* flags,
                         double* fvals, chebgcn_stream stream);
int chebgcn_sym_congruence(const double* W, const double* A, int S, int R, double* out, double* scratch, chebgcn_stream stream);
int chebgcn_sym_mean(const double* matrices, const int32_t* flags, int S, int R, int first, int n_total, double* acc, double* mean,
                     double* norm, chebgcn_stream stream);

/* ---- cross-validated ridge encoding models: every fold and penalty scored from per-run statistics (encoding.ridge_cv) ------------
 * The caller centres every run's features on the host, Xc_r float64 [T_r][F], and forms the per-run statistics with
 * chebgcn_glm_project over the table [Xc_r | 1] (as many calls of at most 64 columns as F + 1 needs):
 *   c      float64 [R][F][Mp]   c[r][j][m] = sum_t Xc_r[t][j] y_r[t][m], Mp = chebgcn_plane_stride(M)
 *   tss    float64 [R][Mp]      tss_r = yy_r - s_r s_r / T_r (s_r the ones column), 0 where below 4 (T_r + 1) 2^-53 yy_r
 * A MODEL e is a training list and a held-out list of runs: list_ptr int32 [2 E + 1], list 2 e = the training runs of model e,
 * list 2 e + 1 its held-out runs, list l = list_runs[list_ptr[l] .. list_ptr[l + 1]) (int32 [nlist], run numbers of c and tss, the
 * caller lists them ascending).  Per model the caller hands, from G_tr = sum Xc_r^T Xc_r = V diag(lambda) V^T and G_te likewise,
 *   V      float64 [E][F][F]    V[j][i] = component j of eigenvector i
 *   H      float64 [E][F][F]    (V^T G_te V + its transpose) / 2: symmetric BIT FOR BIT; the kernel reads H[j][i] where the chain
 *                               below says H[i][j] (row j is contiguous in i), which is the same number only then
 *   d      float64 [E][A][F]    d[a][j] = 1 / (max(lambda_j, 0) + alpha_a), or 0: the kernels never divide by a penalty
 *   Vt     float64 [E][F][F]    Vt[j][i] = V[i][j] (ridge_weights)
 * Every entry of list_ptr is clamped into [0, nlist], a descending pair is an empty list, a list is cut after
 * chebgcn_ridge_query(4) = 64 entries, a run number outside [0, R) is skipped; fold_ptr is clamped into [0, Ef]; a model number of
 * all_model outside [0, E) gives weights of zero; alpha_index is clamped into [0, A): nothing read from memory is an address or a
 * trip count unchecked.  Float64 throughout; EVERY multiply, add, divide and square root is rounded on its own (no fused
 * multiply-add), every chain starts from 0 and runs over ascending index; no float atomics.  A (model, vertex) result is the same
 * bits whatever M, E and the other models are, from call to call.  What the pad columns [M, Mp) of c, tss and the workspace hold
 * (NaN included) is never read; the pad of the workspace and of fold_scores is written as zero.
 *
 * ridge_rotate, per (model e, vertex m):  ct_j = sum_{r in train(e), list order} c[r][j][m],  cs_j likewise over test(e),
 *     z_i = sum_j V[j][i] ct_j,   g_i = sum_j V[j][i] cs_j     (acc = acc + V[j][i] * ct_j over ascending j)
 *   workspace: float64 [E][2][F][Mp], z then g of every model, chebgcn_ridge_workspace(E, F, M) bytes, 8-byte aligned.  The
 *   statistics are read once per (model, list).  chebgcn_last_dispatch(): ridge_rotate_kernel.
 * ridge_score, per (fold model e < Ef, vertex m), from the workspace ridge_rotate left for E >= Ef models:
 *     tss = sum_{r in test(e), list order} tss[r][m]
 *     per penalty a:  w_i = d[a][i] * z_i;   p = sum_i w_i * g_i;   h_i = sum_j H[i][j] * w_j;   q = sum_i w_i * h_i
 *     kind CHEBGCN_RIDGE_R2:  rss = (tss - 2 p) + q;  value = tss > 0 ? 1 - rss / tss : 0
 *     kind CHEBGCN_RIDGE_R:   value = (tss > 0 && q > 0) ? p / sqrt(tss * q) : 0          (never NaN for finite input)
 *   fold_scores float64 [Ef][A][Mp] (scratch of the call, 8-byte aligned).  Then per (subject s, vertex m), the folds of subject s
 *   being the models fold_ptr[s] .. fold_ptr[s + 1] - 1 (int32 [S + 1]), n of them:
 *     mean_a = (sum over the folds in ascending order of value) / n  (0 where n = 0);   a* = the first a that attains the maximum
 *     (scanned upwards with a strict >);   score[s][m] = (float)mean_a*, alpha_index[s][m] = a*, scores[s][a][m] = (float)mean_a.
 *   score float32 [S][M], alpha_index int32 [S][M], scores float32 [S][A][M] or NULL: dense, no pad.
 *   chebgcn_last_dispatch(): ridge_score_kernel<FB> + ridge_select_kernel, FB = chebgcn_ridge_query(100 + F) the bucket of F (64,
 *   128 or 256).
 * ridge_weights, per (subject s, vertex m), e = all_model[s] (int32 [S]: the model whose training list is all the subject's runs),
 *   a = alpha_index[s][m]:   t_j = d[a][j] * z_j;   w_i = sum_j Vt[j][i] * t_j;   weights[s][i][m] = (float)w_i, float32 [S][F][M]
 *   dense.  chebgcn_last_dispatch(): ridge_weights_kernel.
 * ridge_query: 0 vertices of a workgroup, 1 outputs of a register block, 2 the largest F, 3 the largest A, 4 runs of a list at most,
 *   5 models / subjects of one call, 6 threads of a workgroup, 100 + F the score kernel's bucket of F; -1 otherwise.
 * ridge_workspace: bytes for E models (0: arguments out of range).
 * Limits: F <= 256, A <= 32, E <= 65535, S <= 65535: CHEBGCN_EUNSUPPORTED beyond, before any launch, as every CHEBGCN_EINVAL (NULL,
 * counts <= 0, Ef > E, an unknown kind, a workspace too small, a pointer not aligned to its element).  The calls neither
 * synchronise nor allocate. */
enum {
    CHEBGCN_RIDGE_R2 = 0,
    CHEBGCN_RIDGE_R = 1
};
int chebgcn_ridge_query(int what);
size_t chebgcn_ridge_workspace(int E, int F, int M);
int chebgcn_ridge_rotate(const double* c, int R, const int32_t* list_ptr, const int32_t* list_runs, int nlist, const double* V, int E,
                         int F, int M, double* workspace, size_t workspace_bytes, chebgcn_stream stream);
int chebgcn_ridge_score(const double* workspace, size_t workspace_bytes, const double* tss, int R, const int32_t* list_ptr,
                        const int32_t* list_runs, int nlist, const double* H, const double* d, const int32_t* fold_ptr, int E, int Ef,
                        int S, int F, int A, int M, int kind, double* fold_scores, float* score, int32_t* alpha_index, float* scores,
                        chebgcn_stream stream);
int chebgcn_ridge_weights(const double* workspace, size_t workspace_bytes, const double* Vt, const double* d, const int32_t* all_model,
                          const int32_t* alpha_index, int E, int S, int F, int A, int M, float* weights, chebgcn_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* CHEBGCN_H */
