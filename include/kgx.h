/*
 * kgx.h — C-ABI of the MI355X-native message-passing aggregation engine.
 *
 * This is the drop-in boundary for keras-geometric's MessagePassing.propagate()
 * hot path (edge-index gather -> message -> segment-{sum,mean,max,min,std}
 * scatter).  Every entry point takes plain device pointers, sizes and a HIP
 * stream (passed as an opaque pointer so callers need no HIP headers), returns
 * an int status (KGX_OK == 0) and never allocates or frees memory: buffers are
 * owned by the caller (the torch caching allocator in the Python host layer).
 * On failure kgx_last_error() returns a thread-local message.
 *
 * Reference citations are relative to the keras-geometric snapshot the survey
 * studied (src/keras_geometric/...).  The reference itself is pure Python on
 * Keras-3 ops; each function below names the reference code it replaces.
 *
 * Conventions
 *   - node features are fp32, row-major, leading dimension `ld_*` in elements;
 *   - edge ids / node ids are int32 (the reference casts edge_index to int32:
 *     layers/message_passing.py:265, layers/gcn_conv.py:307);
 *   - E (edges) must be < 2^31 - n_dst; feature offsets are computed in int64.
 */
#ifndef KGX_H_
#define KGX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* kgx_stream_t; /* a hipStream_t; NULL = the null stream */

enum kgx_status {
  KGX_OK = 0,
  KGX_ERR_ARG = 1,         /* bad sizes / null pointers / misalignment      */
  KGX_ERR_HIP = 2,         /* HIP runtime error (launch, memcpy, ...)        */
  KGX_ERR_INDEX = 3,       /* an edge index lies outside the node range      */
  KGX_ERR_UNSUPPORTED = 4  /* shape the kernels do not implement             */
};

/* Segment reductions: layers/aggregators.py Sum(:119-141) Mean(:48-89)
 * Max(:92-116) Min(:144-171) Std(:174-232).                                  */
enum kgx_reduce { KGX_SUM = 0, KGX_MEAN = 1, KGX_MAX = 2, KGX_MIN = 3, KGX_STD = 4 };

/* Fused epilogues applied after the reduction of a destination row.
 *   BIAS: out = aggr + bias[f]              (GCNConv.update, gcn_conv.py:266-272)
 *   GIN : out = gin_scale * x[row,f] + aggr (GINConv.update, gin_conv.py:216-222)
 *   RAW : MAX / MIN without the aggregators' isinf -> 0 guard: plain
 *         keras.ops.segment_max semantics (empty segment -> -inf), as
 *         BatchGlobalPooling uses it (global_pooling.py:228-249)            */
/* KGX_EPI_ACCUM (reduce KGX_SUM only): out[row] += this launch's row sum, read
 * from and written to `out` in place -- the sharded GIN / SAGE halo-chunk
 * passes (no reference counterpart; distributed.py). */
enum kgx_epilogue { KGX_EPI_NONE = 0, KGX_EPI_BIAS = 1, KGX_EPI_GIN = 2, KGX_EPI_RAW = 3, KGX_EPI_ACCUM = 4 };

/* Graph-preparation flags. */
enum kgx_csr_flags {
  KGX_CSR_SELF_LOOPS = 1, /* append (i,i) after the E input edges: utils/main.py:8-16    */
  KGX_CSR_SEGMENT_ONLY = 2, /* segment semantics only (Aggregator.aggregate called directly,
                               aggregators.py:24-39): ids outside [0,n_dst) are dropped,
                               src is not validated                                       */
  KGX_CSR_GCN_NORM = 4    /* also produce dinv[n_dst] and per-CSR-edge weight w:
                               utils/main.py:20-33                                        */
};

int kgx_version(void);
const char* kgx_last_error(void);

/* ---------------------------------------------------------------------------
 * The CU split (KGX_FUSED_CU_SPLIT launches): validated on gfx950 with 256 CUs
 * in 8 XCDs only.  kgx_cu_split_layout_ok: 1 when (cus, xccs, arch) is that
 * layout (pure, no device needed).  kgx_cu_split_supported: 1 when `device`
 * has it, 0 when its KGX_FUSED_CU_SPLIT launches run unsplit (one note on
 * stderr), < 0 on error.  A launch whose stream is on another device than the
 * current one also runs unsplit.
 * ------------------------------------------------------------------------- */
int kgx_cu_split_layout_ok(int cus, int xccs, const char* arch);
int kgx_cu_split_supported(int device);
/* Census of the CU-masked streams a split launch uses (a diagnostic the tests run):
 * n_blocks short blocks on the head stream and n_blocks on the tail stream of
 * cu_split(per32) each record where they ran, (XCC id << 8) | (SE id << 5) |
 * (SH id << 4) | CU id from the hardware registers, into head_ids[n_blocks] and
 * tail_ids[n_blocks]; n_cus[0] / n_cus[1] = the head / tail CU counts the split
 * believes its masks hold.  Synchronises the caller's stream.  KGX_ERR_UNSUPPORTED
 * when the device has no validated split layout.  Checks that the masks are
 * disjoint and cover what they claim (tests/test_gpu_cu_census.py). */
int kgx_cu_split_census(int per32, int64_t n_blocks, int32_t* head_ids, int32_t* tail_ids, int* n_cus,
                        kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Graph preparation: COO int32 [2,E] (generation order, unsorted) -> CSR by
 * destination, STABLE (edges of one destination keep their input order, the
 * self-loop is last), which is the order the reference's segment_sum
 * (Keras-torch scatter_add) accumulates in.
 *
 * Replaces: MessagePassing.call edge_index cast/cache (message_passing.py:256-268),
 *           add_self_loops (utils/main.py:8-16), the degree segment_sum of
 *           compute_gcn_normalization (utils/main.py:23-24) and of
 *           MeanAggregator (aggregators.py:66-69).
 *
 * Index semantics (Keras-3 torch lowering of take/segment_sum):
 *   src in [-n_src, n_src): negative ids wrap (+n_src), else KGX_ERR_INDEX;
 *   dst in [-n_dst, n_dst): negative ids are dropped from every segment
 *   reduction (and from degrees), else KGX_ERR_INDEX.
 *   With KGX_CSR_SEGMENT_ONLY every dst outside [0,n_dst) is dropped.
 * Outputs (caller-allocated, capacity E + n_dst when SELF_LOOPS else E):
 *   rowptr[n_dst+1], col[cap] (source id per CSR slot), eid[cap] (input edge
 *   id per CSR slot; self loop i has id E+i), deg[n_dst] (int32 in-degree),
 *   optional dinv[n_dst] and w[cap] (KGX_CSR_GCN_NORM).
 * KGX_ERR_ARG: SELF_LOOPS or GCN_NORM with n_src != n_dst (w indexes the one
 *   dinv[n_dst] table with the source id; a bipartite graph takes
 *   kgx_gcn_edge_norm with dinv_dst / dinv_src), and GCN_NORM together with
 *   SEGMENT_ONLY (whose sources are neither range-checked nor wrapped).
 * info[4] (host) receives: kept edges, max in-degree, #bad indices, and
 * (kgx_csr_build2) the rows whose degree the dinv table did not cover.
 * This call synchronises `stream` once (to return info).
 *
 * GCN_NORM's dinv: kgx_csr_build computes (deg + 1e-12)^-0.5 correctly
 * rounded.  kgx_csr_build2 takes it from the caller's device table instead,
 *   dinv[i] = dinv_table[min(deg[i], 2^24)],   table_len entries,
 * filled with the reference's own values: utils/main.py:25's
 * power(deg + 1e-12, -0.5) lowers to torch.pow(Tensor, Tensor), ATen's
 * vectorised (Sleef) powf, which differs from the correctly-rounded value by
 * 1 ulp for some degrees.  With that table dinv and w are bit-identical to
 * the reference's (graph.gcn_dinv_table builds it).  A degree the table does
 * not cover takes the correctly-rounded value and is counted in info[3]; the
 * caller then redoes dinv / w with a longer table (kgx_gcn_dinv_table +
 * kgx_gcn_edge_norm).  dinv_table NULL: kgx_csr_build.
 * ------------------------------------------------------------------------- */
int kgx_csr_workspace_bytes(int64_t E, int64_t n_dst, int flags, size_t* bytes);
int kgx_csr_build(const int32_t* src, const int32_t* dst, int64_t E,
                  int64_t n_src, int64_t n_dst, int flags,
                  int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* deg,
                  float* dinv, float* w,
                  void* workspace, size_t workspace_bytes,
                  int64_t* info, kgx_stream_t stream);
int kgx_csr_build2(const int32_t* src, const int32_t* dst, int64_t E,
                   int64_t n_src, int64_t n_dst, int flags,
                   int32_t* rowptr, int32_t* col, int32_t* eid, int32_t* deg,
                   float* dinv, float* w, const float* dinv_table, int64_t table_len,
                   void* workspace, size_t workspace_bytes,
                   int64_t* info, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Schedule tails, on the device (the fused kernels' short-row and tiny-row
 * launches take the degree-descending schedule's suffix of small unsplit rows):
 * kgx_schedule_suffixes: out[0] = 1 + the last item (int4 {row, beg, end,
 * slot}) that is split or has more than short_max edges, out[1] the same for
 * tiny_max (0: none).  kgx_tiny_pack: the records of items [start, start+n):
 * pack[i] = {row, degree, col0, col1} (col1 = col0 for degree 1, 0 / 0 for
 * degree 0; indices clamped to n_col - 1), tw[i] = {w0, w1} (0 where absent;
 * tw NULL: unweighted); out[0] = records of degree 2, out[1] = 1 + the last
 * of them.  Both take a 16-byte device workspace and synchronise `stream`.
 * ------------------------------------------------------------------------- */
int kgx_schedule_suffixes(const int32_t* items, int64_t n_items, int short_max, int tiny_max,
                          void* workspace, int64_t* out, kgx_stream_t stream);
int kgx_tiny_pack(const int32_t* items, int64_t start, int64_t n, const int32_t* col, const float* w,
                  int64_t n_col, int32_t* pack, float* tw, void* workspace, int64_t* out,
                  kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * GCN normalisation for a CSR whose sources index a different table than its
 * rows (a destination-range shard: rows = owned nodes, sources = owned + halo
 * nodes).  Same arithmetic as KGX_CSR_GCN_NORM (utils/main.py:20-33):
 *   dinv[i] = (float(min(deg[i], 2^24)) + 1e-12f)^-0.5  (correctly rounded)
 *   w[e]    = dinv_dst[row(e)] * dinv_src[col[e]]       (CSR order)
 * kgx_gcn_dinv_table: dinv[i] = table[min(deg[i], 2^24)] (the reference's
 * values, see kgx_csr_build2); the caller's table must cover
 * min(max(deg), 2^24) (indices past it read the last entry).
 * ------------------------------------------------------------------------- */
int kgx_gcn_dinv(const int32_t* deg, int64_t n, float* dinv, kgx_stream_t stream);
int kgx_gcn_dinv_table(const int32_t* deg, int64_t n, const float* table, int64_t table_len,
                       float* dinv, kgx_stream_t stream);
int kgx_gcn_edge_norm(const int32_t* rowptr, const int32_t* col, int64_t n_dst,
                      const float* dinv_dst, const float* dinv_src, float* w,
                      kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Row schedule (no reference counterpart: the reference has one device and no
 * scheduling).  Orders destination rows by descending exact degree (stable:
 * ascending row id among equal degrees; degrees >= 2^24 - 1 tie) so hub rows
 * start first, and cuts rows with deg >= split_len into split_len-edge chunks
 * whose partials are combined in chunk order: chunk c of a row [beg, end) is
 * [beg + c*split_len, min(end, beg + (c+1)*split_len)) with slot first_slot + c,
 * and the slots of all split rows are dense in [0, n_slots).
 *   rows[n_dst]              row ids in schedule order (EXACT mode iterates these)
 *   items[4*cap_items]       {row, edge_begin, edge_end, partial_slot|-1}
 *   split[4*n_dst]           {row, first_slot, n_chunks, degree} for split rows
 * cap_items must be >= n_dst + E_kept / split_len + 1.  split_len <= 0 means
 * never split.  info[4] (host): n_items, n_split_rows, n_slots, 0.  Syncs once.
 * ------------------------------------------------------------------------- */
int kgx_schedule_workspace_bytes(int64_t n_dst, size_t* bytes);
int kgx_schedule_build(const int32_t* rowptr, int64_t n_dst, int32_t split_len,
                       int32_t* rows, int32_t* items, int64_t cap_items,
                       int32_t* split, void* workspace, size_t workspace_bytes,
                       int64_t* info, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * kgx_work: one graph's work list -- the CSR, its degree-ordered schedule
 * (kgx_schedule_build) and the packed degree <= 2 tail (tiny.py) -- as the
 * argument structs of kgx_spmm_run ("spmm" below), kgx_spmm_gemm_run ("gemm")
 * and kgx_spmm_gemm_f256_run ("f256") carry it.  Zero / NULL = absent.
 *   rowptr, rows, n_rows   [all] CSR row pointer [n_rows + 1] and the row ids in
 *       schedule order [n_rows].
 *   items, n_items         [all] the (possibly split) item list of
 *       kgx_schedule_build; split rows are finished by an in-call fix-up through
 *       the call's `partials`.  items NULL: every row of `rows` is reduced whole
 *       in CSR order and the schedule's other fields are not used (spmm: EXACT
 *       mode).  KGX_STD ignores items (always EXACT, two sequential passes per row).
 *   n_long_items           [all] where the degree-descending schedule's short
 *       rows begin: items [n_long_items, n_short_end) are unsplit rows of degree
 *       <= KGX_SHORT_ROW_MAX.
 *       spmm: a second kernel takes them several per lane group (not with
 *         message dropout or column slices wider than 64 lanes); must lie in
 *         [0, n_items], n_items = none.  EXACT mode (items NULL): 0 <
 *         n_long_items < n_rows names the same suffix of the degree-descending
 *         `rows` list, rows[n_long_items, n_rows), for the same kernel (each row
 *         still one chain of adds in CSR order: bit-identical); any other value
 *         leaves every row to the main kernel.
 *       gemm: the short-row kernel reduces them 64 rows per block iteration;
 *         0 <= n_long_items <= n_short_end <= n_items, n_short_end = none.  With
 *         a sliced schedule it is the kgx_slice_build call's n_long_items.
 *       f256: items [0, n_short_end) go to the main kernel, as two launches when
 *         0 <= n_long_items < n_short_end (the hub chunks and rows of degree >
 *         KGX_SHORT_ROW_MAX first, then the short rows, gathered whole a tile
 *         ahead); -1: one launch.
 *   n_short_end            [gemm, f256] items [n_short_end, n_items), rows of
 *       degree <= 2, are taken from tiny_pack instead of the item list.  tiny_pack
 *       NULL, and always in spmm (no tiny-record path): must equal n_items.
 *   tiny_pack, tiny_w      [gemm, f256; spmm: must be NULL] the packed tail,
 *       built once per graph (tiny.py, kgx_tiny_pack): tiny_pack[n_items -
 *       n_short_end][4] = {row, degree, col0, col1} (col1 = col0 for degree 1,
 *       both any valid source for degree 0) and, when w is given, tiny_w[..][2]
 *       = {w0, w1}.  Needs items.
 *   n_tiny_deg2            [gemm] the first n_tiny_deg2 records have degree 2
 *       (the rest <= 1: degree-descending order); in [0, n_items - n_short_end].
 *   split, n_split         [all] {row, first_slot, n_chunks, degree} of the
 *       split rows; n_split > 0 needs split and the call's partials.
 *   idx, w                 [all] per CSR slot the gathered row (col, or eid for
 *       a per-edge message tensor) and, optional, the edge weight.
 * ------------------------------------------------------------------------- */
enum { KGX_SHORT_ROW_MAX = 7 };
typedef struct kgx_work {
  const int32_t* rowptr; const int32_t* rows; int64_t n_rows;
  const int32_t* items;  int64_t n_items; int64_t n_long_items; int64_t n_short_end;
  const int32_t* tiny_pack; const float* tiny_w; int64_t n_tiny_deg2;
  const int32_t* split;  int64_t n_split;
  const int32_t* idx;    const float* w;
} kgx_work;

/* ---------------------------------------------------------------------------
 * Fused gather -> (weight) -> segment reduction -> epilogue, one launch.
 *   out[row, f] = EPI( REDUCE_{e in CSR row} table[idx[e], f] * (w ? w[e] : 1) )
 *
 * Replaces: MessagePassing.propagate's take(x_j, src) (message_passing.py:195),
 *   the default/GCN/GIN/SAGE message (message_passing.py:73-77, gcn_conv.py:233-248,
 *   gin_conv.py:193, sage_conv.py:294-298), MessagePassing.aggregate ->
 *   Aggregator.aggregate (message_passing.py:79-102, aggregators.py:48-232) and
 *   the GCN/GIN update epilogues.
 * With idx = col and table = node features it is the node-gather SpMM; with
 *   idx = eid and table = a per-edge message tensor [E,F] it is the reference's
 *   Aggregator.aggregate(messages, target_idx, dim_size) on arbitrary messages.
 *
 * kgx_spmm_run takes its arguments as a kgx_spmm_args (zero-fill it, then set
 * the fields the launch needs):
 *   struct_size   sizeof(kgx_spmm_args), else KGX_ERR_ARG (a binding of another header).
 *   reduce, epilogue   a kgx_reduce and a kgx_epilogue.  EPI_BIAS needs bias,
 *       EPI_GIN xroot with ld_x >= F, EPI_ACCUM reduce KGX_SUM.
 *   work          the work list (kgx_work; no tiny records).  items NULL is EXACT
 *       mode: each row one sequential reduction in CSR order, bit-identical to the
 *       reference's sequential scatter_add / scatter_reduce for identical messages.
 *   table, ld_table, F   the gathered table [*, ld_table >= F], ld_table < 2^31.
 *   table2, n_table1   gather from TWO tables: sources c < n_table1 are rows of
 *       table, c >= n_table1 rows c - n_table1 of table2 (same ld_table); 0 <=
 *       n_table1 < 2^31.  Needs the schedule (items; not EXACT / std), plain or
 *       weighted KGX_SUM, no dropout.  The sharded GIN / SAGE layers reduce a
 *       row's own-source and halo edges in one pass (distributed.py;
 *       gin_conv.py:216-222, sage_conv.py:300-348).  table2 NULL: one table.
 *   out, ld_out   [n_rows, ld_out >= F].
 *   bias, xroot, ld_x, gin_scale   the epilogues' operands (kgx_epilogue).
 *   drop_key, drop_p, drop_seed   (optional, SUM only, 0 <= p < 1) per-slot keys
 *       of the message dropout mask (see kgx_dropout_mask); the message is
 *       (table[idx] * mask) * w.
 *   partials      n_slots * F floats, needed when the schedule has split rows.
 *   counters      EXACT mode only (ignored with items): two caller-owned int32,
 *       zeroed before the call, from which the hub-row kernel (rows of >= 2048
 *       edges) hands out its (row, column group) items dynamically, so its
 *       blocks balance instead of waiting behind the largest row (bit-identical
 *       results: every row is still reduced by one lane chain in CSR order,
 *       aggregators.py:126-137).  NULL: the static schedule.  With counters the
 *       hub kernel also forks onto a library-owned stream beside the main
 *       kernel (joined back into `stream` before the call returns), and the
 *       main kernel takes interleaved batches of rows from counters[1] (batch b
 *       = rows b, b + NB, ..., one atomic per 8 rows), so the GPU is not idle
 *       behind the largest hub row (KGX_EXACT_FORK=0: the sequential form).
 * kgx_spmm is the minimal positional form: kgx_spmm_run with n_long_items =
 * n_short_end = n_items, one table and no counters.
 * ------------------------------------------------------------------------- */
typedef struct kgx_spmm_args {
  uint64_t struct_size;
  int32_t reduce, epilogue;
  kgx_work work;
  const float* table; int64_t ld_table; const float* table2; int64_t n_table1; int64_t F;
  float* out; int64_t ld_out;
  const float* bias; const float* xroot; int64_t ld_x; float gin_scale; float drop_p;
  const int32_t* drop_key; uint64_t drop_seed;
  float* partials; int32_t* counters;
} kgx_spmm_args;
int kgx_spmm_run(const kgx_spmm_args* a, kgx_stream_t stream);
int kgx_spmm(int reduce, int epilogue,
             const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
             const int32_t* items, int64_t n_items,
             const int32_t* split, int64_t n_split,
             const int32_t* idx, const float* w,
             const float* table, int64_t ld_table, int64_t F,
             float* out, int64_t ld_out,
             const float* bias, const float* xroot, int64_t ld_x, float gin_scale,
             const int32_t* drop_key, float drop_p, uint64_t drop_seed,
             float* partials, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused multi-aggregation: several reducers of one neighbourhood from ONE
 * gather of every neighbour row (no reference counterpart as a whole; each
 * block is kgx_spmm's single-reducer arithmetic, aggregators.py:48-232).
 *   out[row, k*F + f] = REDUCE_{reduces[k]} { table[idx[e], f] : e in CSR row }
 * reduces: host array of n_red (1..5) distinct kgx_reduce ids; the blocks are
 *   concatenated along the feature axis in that order (ld_out >= n_red * F),
 *   the layout a following Dense wants.  No edge weights, dropout or epilogues.
 * With idx = col it is the node gather; with idx = eid and table = a per-edge
 *   message tensor [E,F] it reduces arbitrary messages.
 * Work list, as kgx_spmm: items == NULL is EXACT mode (every row of `rows`
 *   reduced by one lane group in CSR order: each block bit-identical to
 *   kgx_spmm's EXACT result, KGX_STD included); otherwise the item list of
 *   kgx_schedule_build.  Unsplit items are reduced with the EXACT arithmetic;
 *   a chunk of a split row writes its raw state to `partials` and a fix-up
 *   kernel folds each row's chunks in chunk order (no atomics: results are
 *   bit-identical from run to run).  Unlike kgx_spmm, KGX_STD follows the
 *   schedule too: a chunk keeps M2 = sum (v - chunk_mean)^2 and its length,
 *   merged pairwise as M2 = M2a + M2b + d^2 na nb / (na + nb), d = mean_b - mean_a
 *   (a re-association of the two-pass form on split rows only).
 * partials: per slot one section of F floats for each accumulator the list
 *   needs, in the order {sum (sum | mean | std), amax (max), amax of -m (min),
 *   M2 (std)}, then with std 4 floats whose first is the chunk length.
 *   kgx_multi_aggr_partials_floats gives n_slots times that; partials_floats
 *   is the buffer's size in floats (chunk stores past it are dropped).
 * KGX_ERR_ARG (before any device work, nothing written): null reduces / rowptr /
 *   rows / idx / table / out, n_red outside 1..5, an unknown or repeated id,
 *   negative sizes, ld_out < n_red*F, ld_table < F or >= 2^31, split rows
 *   without split list or partials, partials_floats below one slot per split row.
 * ------------------------------------------------------------------------- */
int kgx_multi_aggr(int n_red, const int* reduces,
                   const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                   const int32_t* items, int64_t n_items,
                   const int32_t* split, int64_t n_split,
                   const int32_t* idx, const float* table, int64_t ld_table, int64_t F,
                   float* out, int64_t ld_out,
                   float* partials, int64_t partials_floats,
                   kgx_stream_t stream);
int kgx_multi_aggr_partials_floats(int n_red, const int* reduces, int64_t n_slots, int64_t F, int64_t* floats);

/* Message dropout mask (training; GCNConv.message dropout, gcn_conv.py:237-242;
 * GATv2 attention dropout, gatv2_conv.py:252-253): element (key, f) is kept
 * with probability 1 - p and scaled by 1/(1-p).  The mask is a pure function
 * of (seed, key = input edge id, f), so a layer's forward (kgx_spmm with
 * drop_key = the CSR's input edge ids), its backward over the transposed
 * graph and tests agree.  kgx_dropout_mask writes the multiplier (0 or
 * 1/(1-p)) of n keys x F columns, row-major. */
int kgx_dropout_mask(uint64_t seed, float p, const int32_t* keys, int64_t n, int64_t F, float* out,
                     kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused aggregate -> dense transform (+ bias), one launch (plus a fix-up for
 * split hub rows):
 *   out[i,:] (+)= bias + PRE( REDUCE_{e in row i} x[idx[e],:] * (w ? w[e] : 1) ) @ W
 *   PRE = identity, or gin_scale * x[i,:] + aggr with KGX_FUSED_PRE_GIN;
 *   "+=" (read-add-write of out) with KGX_FUSED_ACCUMULATE, used to add the
 *   halo-source part of a sharded row after its local part (distributed.py),
 *   and SAGEConv's neighbour map onto out = b + x W_self (sage_conv.py:404-433).
 * Replaces GCNConv's per-edge x_j @ W + segment_sum + bias (gcn_conv.py:233-272)
 * and GINConv's (1+eps)x + aggr -> single-Dense MLP (gin_conv.py:216-225) by the
 * algebraically equal aggregate-then-transform order (W applied once per row
 * on MFMA as the six significant products of a three-way bf16 split of both
 * operands: f32-accurate); tolerance-equal to the reference, not bit-equal.
 * Two calls take one kgx_fused_args (below): kgx_spmm_gemm_run for F_in <= 128
 * and kgx_spmm_gemm_f256_run for 256-wide rows -- GINConv's (1+eps) x + aggr ->
 * Dense at BASELINE config C4 (gin_conv.py:216-225, 129-162) and GCNConv 256 ->
 * 256 (gcn_conv.py:233-272) without the [N, 256] aggregate written and read back.
 * kgx_spmm_gemm is the minimal positional form of kgx_spmm_gemm_run.
 * ------------------------------------------------------------------------- */
/* KGX_FUSED_SHARE_GPU: launch (den - 1) / den of the resident grid (den =
 * KGX_SHARE_DEN, default 16; the 256-wide kernels take the flag and ignore it), leaving block slots
 * for kernels of a concurrent stream (the sharded layer's RCCL exchange).
 * KGX_FUSED_RELU: out = max(bias + ..., 0), the activation of a GIN MLP's
 * first Dense (gin_conv.py:129-162) or SAGEConv's activation; with ACCUMULATE
 * it applies to the sum (out = max(out + ..., 0)).  kgx_spmm_gemm_f256_run
 * rejects RELU | ACCUMULATE. */
/* KGX_FUSED_CU_SPLIT: run the schedule's tail launches on a CU-masked stream
 * over 8 of every 32 CUs, beside the main launches on the other CUs; both
 * streams are forked from and joined back into `stream` (before the hub
 * fix-up).  Outputs are bit-identical to the one-stream order.
 * kgx_spmm_gemm_f256_run: the tail is the degree <= 2 records (MFMA-bound),
 * the main part the long rows and degree 3..7 (memory-bound);
 * KGX_F256_CU_SPLIT (environment) = tail CUs per 32, 0 = ignore the flag.
 * kgx_spmm_gemm, kgx_spmm_gemm_run: the tail is the short-row and tiny-record
 * launches, the main part spmm_gemm_kernel; KGX_FUSED_CU_SPLIT (environment) =
 * tail CUs per 32. */
enum { KGX_FUSED_PRE_GIN = 1, KGX_FUSED_ACCUMULATE = 2, KGX_FUSED_SHARE_GPU = 4, KGX_FUSED_RELU = 8,
       KGX_FUSED_CU_SPLIT = 16 };
int kgx_spmm_gemm(int reduce, const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                  const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                  const int32_t* idx, const float* w, const float* x, int64_t ld_x, int64_t F_in,
                  const float* W, int64_t F_out, const float* bias, int flags, float gin_scale,
                  float* out, int64_t ld_out, float* partials, float* agg_out, int64_t ld_agg,
                  kgx_stream_t stream);

/* Sliced schedule of the fused launch (kgx_fused_args.slice): rows of degree >= T
 * (the split hub rows among them; T <= split_len) have their edges regrouped by
 * SOURCE CLASS, a hash of the source id into [0, C): kgx_slice_class below.
 * Each XCD's L2 then holds one class of the hot source rows instead of a copy
 * of all of them.  Built once per reused graph, beside the schedule:
 *   kgx_slice_count: info[0] = rows of degree >= T, info[1] = their edges,
 *     info[2] = their items (a prefix of the degree-descending item list; only
 *     items [0, n_long_items) are looked at).  ws: 32 bytes.  Syncs once.
 *   kgx_slice_build, for rows[0, n_rows_s) (that prefix of the schedule's row
 *     order) with n_edges_s edges and items [0, n_items_s):
 *       col_s / w_s [n_edges_s]  the rows' edges, row by row in schedule order,
 *                                each row grouped by class, CSR order kept
 *                                inside a class (stable sort; w NULL: no w_s)
 *       items_s [cap_items][4]   C item lists back to back.  List c: the class-c
 *                                chunks {row, beg, end, slot} (offsets into
 *                                col_s, <= split_len edges, slot >= 0), rows in
 *                                schedule order, then its share of items
 *                                [n_items_s, n_long_items) of the item list,
 *                                copied in 16-item tiles dealt round-robin
 *       lists [C][4]             {first item, items, chunk items, 0} of list c
 *       fix [n_rows_s][4]        {row, first slot, slots, degree}; a row's slots
 *                                are consecutive, in class then chunk order
 *     cap_items >= n_edges_s / split_len + n_rows_s * C + n_long_items - n_items_s.
 *     info[0] = items in all lists, info[1] = slots, info[2] = items of the
 *     longest list, info[3] = chunk items.  Deterministic.  Syncs once.
 * kgx_slice_class: the class of source id `col` (host, pure).
 * kgx_slice_grid: the grid of a sliced launch, a multiple of n_classes within
 *   resident_blocks, at most list_tiles blocks per list; 0 = run unsliced. */
int kgx_slice_class(int32_t col, int n_classes);
int kgx_slice_grid(int64_t resident_blocks, int64_t list_tiles, int n_classes);
int kgx_slice_count(const int32_t* rowptr, int64_t n_dst, const int32_t* items, int64_t n_long_items, int32_t T,
                    void* ws, int64_t* info, kgx_stream_t stream);
int kgx_slice_workspace_bytes(int64_t n_rows_s, int64_t n_edges_s, int n_classes, size_t* bytes);
int kgx_slice_build(const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rows,
                    int64_t n_rows_s, int64_t n_edges_s, const int32_t* items, int64_t n_items_s,
                    int64_t n_long_items, int32_t split_len, int n_classes, int32_t* col_s, float* w_s,
                    int32_t* items_s, int64_t cap_items, int32_t* lists, int32_t* fix, void* workspace,
                    size_t workspace_bytes, int64_t* info, kgx_stream_t stream);

/* kgx_slice: a sliced schedule (kgx_slice_build) for kgx_spmm_gemm_run's main
 * kernel.  kgx_spmm_gemm_f256_run has none: n_classes must be 0 there.
 *   n_classes     0 = unsliced, nothing else is read; else 4 or 8 lists, block b
 *       of the main kernel on list b % n_classes -- an XCD affinity label only:
 *       every item is reduced once by a statically determined block, and
 *       results do not depend on where blocks run.  Rows that are not sliced
 *       get bit-identical results either way.  Needs work.items and partials;
 *       unweighted or weighted sums, one table, F_in 128, F_out % 16 == 0
 *       (anything else: KGX_ERR_UNSUPPORTED).  When no multiple of n_classes
 *       blocks fits the launch (kgx_slice_grid), it runs unsliced from
 *       work.items / work.split.
 *   items, lists  kgx_slice_build's items_s and lists.
 *   tiles         ceil(longest list / 16), > 0.
 *   idx, w        col_s / w_s, the sliced rows' regrouped edges (w needed with work.w).
 *   split, n_split   the `fix` records, n_split > 0; they replace work.split /
 *       work.n_split.  The sliced rows' chunks write partials: n_slots of
 *       kgx_slice_build * 128 floats, and `partials` must hold the larger of
 *       the two schedules' slots.
 *   head_short_end   (<= work.n_short_end; anything <= work.n_long_items: none)
 *       under KGX_FUSED_CU_SPLIT the short-row items [n_long_items,
 *       head_short_end) run on the head's CUs behind the main kernel, by the
 *       short-row kernel, and the tail's CUs take the rest -- the knob that
 *       rebalances the two legs once slicing has shortened the head. */
typedef struct kgx_slice {
  const int32_t* items; const int32_t* lists; int64_t n_classes; int64_t tiles;
  const int32_t* idx; const float* w; const int32_t* split; int64_t n_split;
  int64_t head_short_end;
} kgx_slice;

/* kgx_fused_args, read by kgx_spmm_gemm_run ("gemm") and kgx_spmm_gemm_f256_run
 * ("f256"); both read every field but `slice` (zero-fill the struct first):
 *   struct_size   sizeof(kgx_fused_args), else KGX_ERR_ARG.
 *   reduce, flags KGX_SUM, MEAN, MAX or MIN; KGX_FUSED_* (unknown bits: KGX_ERR_ARG).
 *   work          the work list (kgx_work), short rows and tiny records included: the
 *       positional call's boundary (gcn_conv.py:233-272, aggregators.py:56-167).
 *   x, ld_x       the feature table, 16-byte aligned, ld_x % 4 == 0, ld_x in
 *       [F_in, 2^31).  KGX_FUSED_PRE_GIN's root rows are rows of x.
 *   x2, n_x1      gather from TWO feature tables: source columns c < n_x1 are
 *       rows of x, columns c >= n_x1 rows c - n_x1 of x2 (same ld_x, 16-byte
 *       aligned; 0 <= n_x1 < 2^31).  The sharded layers' halo pass reads a
 *       row's own-source edges from the layer input and its halo edges from
 *       the exchange's receive buffer in ONE pass, so the row is written once
 *       instead of written and read-modify-written (distributed.py;
 *       gcn_conv.py:233-272, gin_conv.py:216-225 per shard).  With x2: sums
 *       only (weighted or not, GIN's pre-scale allowed); gemm also needs F_in
 *       128 and F_out % 16 == 0 (else KGX_ERR_UNSUPPORTED).  x2 NULL: one table.
 *   F_in, W, F_out   W [F_in, F_out] row-major.  gemm: F_in and F_out multiples
 *       of 4 <= 128.  f256: F_in == 256, F_out a multiple of 16 <= 256.
 *   bias, gin_scale   [F_out], optional; KGX_FUSED_PRE_GIN's factor.  pad_ is not read.
 *   out, ld_out   [n_rows, ld_out >= F_out], 16-byte aligned, ld_out % 4 == 0 (dwordx4 stores).
 *   partials      one slot per hub chunk of n_slots, gemm 128 floats per slot,
 *       f256 256; needed when the schedule has split rows or is sliced.
 *   agg_out, ld_agg  (optional, [n, ld_agg >= F_in], 16-byte aligned, ld_agg % 4
 *       == 0) also store PRE(REDUCE(...)), the rows before the transform --
 *       what the backward's dW = agg^T dOut needs.
 *   slice         [gemm] the sliced schedule (kgx_slice); [f256] n_classes must be 0.
 * Both fail with KGX_ERR_ARG / KGX_ERR_UNSUPPORTED before any device work. */
typedef struct kgx_fused_args {
  uint64_t struct_size;
  int32_t reduce, flags;
  kgx_work work;
  const float* x; int64_t ld_x; const float* x2; int64_t n_x1; int64_t F_in;
  const float* W; int64_t F_out; const float* bias; float gin_scale; float pad_;
  float* out; int64_t ld_out; float* partials; float* agg_out; int64_t ld_agg;
  kgx_slice slice;
} kgx_fused_args;
int kgx_spmm_gemm_run(const kgx_fused_args* a, kgx_stream_t stream);
int kgx_spmm_gemm_f256_run(const kgx_fused_args* a, kgx_stream_t stream);


/* ---------------------------------------------------------------------------
 * Weight and bias gradients of a layer out = P W + b (the fused layers'
 * training step, kgx_dense's backward):
 *   dW[k, m] = sum_n P[n, k] D[n, m]  (K x M, row stride ld_dw)
 *   db[m]    = sum_n D[n, m]          (NULL: not computed)
 * in one pass over P [N, K] and D = dOut [N, M] (row strides ldp, ldd, unit
 * column stride).  bf16x3-split MFMA products (f32-accurate), the node sum
 * split over row ranges and the partials added in a fixed order
 * (deterministic).  A row range holding an inf / NaN is recomputed in plain
 * f32 (IEEE propagation).  Workspace: kgx_gemm_tn_workspace_bytes.
 * Replaces: the reference autograd's matmul / sum backward of
 * gcn_conv.py:233-272 (x_j W, + bias) and of keras Dense (gin_conv.py:129-162,
 * sage_conv.py:404-433).
 * ------------------------------------------------------------------------- */
int kgx_gemm_tn_workspace_bytes(int64_t N, int64_t K, int64_t M, size_t* bytes);
int kgx_gemm_tn(int64_t N, const float* P, int64_t ldp, int64_t K, const float* D, int64_t ldd, int64_t M,
                float* dW, int64_t ld_dw, float* db, void* workspace, size_t workspace_bytes,
                kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of the segment max / min reduction (autograd of kgx_spmm MAX/MIN).
 * torch's scatter_reduce amax/amin backward, under the reference's isinf
 * guard (aggregators.py:99-112, 151-167): grad_out[i,f] is shared evenly by
 * the edges of row i whose message equals the row's raw extreme; rows whose
 * extreme is +-inf (empty rows included) or NaN pass nothing.
 *   grad_table[idx[e], f] += grad_out[i, f] / ties   (float atomics)
 * raw != 0 (KGX_EPI_RAW forward): no guard -- a +-inf extreme shares its
 * gradient with its tied edges, and a -inf extreme also with the -inf init
 * (torch's include_self count).
 * grad_table must be zero-initialised by the caller.  Sum / mean / weighted
 * sums need no separate entry point: their backward is kgx_spmm over the
 * transposed graph (a kgx_csr_build of the reversed edges).
 * ------------------------------------------------------------------------- */
int kgx_spmm_max_backward(int reduce, int raw, const int32_t* rowptr, int64_t n_rows, const int32_t* idx,
                          const float* table, int64_t ld_table, int64_t F,
                          const float* grad_out, int64_t ld_grad_out,
                          float* grad_table, int64_t ld_grad_table, kgx_stream_t stream);
/* The same with edge weights w[slot] (null: none), the backward of a weighted
 * kgx_spmm / kgx_spmm_gemm MAX / MIN: the messages are the forward's fp32
 * products table[idx[e]] * w[e] -- extreme and ties among them -- and
 *   grad_table[idx[e], f] += (grad_out[i, f] / ties) * w[e].
 * raw != 0 takes no weights (KGX_ERR_UNSUPPORTED). */
int kgx_spmm_max_backward_w(int reduce, int raw, const int32_t* rowptr, int64_t n_rows, const int32_t* idx,
                            const float* w, const float* table, int64_t ld_table, int64_t F,
                            const float* grad_out, int64_t ld_grad_out,
                            float* grad_table, int64_t ld_grad_table, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused GATv2 attention aggregation (single pass, online segment softmax).
 *   s[e,h]  = sum_c att[h,c] * leaky_relu(h_dst[i,h,c] + h_src[j,h,c], slope)
 *   alpha   = exp(s - max_i) / (sum_i exp(s - max_i) + 1e-10)
 *   out[i,h,c] = sum_e alpha[e,h] * h_src[j,h,c]  (+ bias[h*C+c] if bias)
 * Replaces GATv2Conv._gatv2_propagate's gathers, _compute_attention,
 *   _softmax_by_target, alpha*h_j, _aggregate_messages and the concat-mode
 *   _final_update (gatv2_conv.py:241-266, 268-311, 313-335, 337-352).
 * h_src/h_dst: [n, heads*channels] row-major with leading dimension ld_h.
 * partials: n_slots * ld_p floats when items are split, ld_p = heads*channels +
 *   2*heads rounded up to a multiple of 4 (each slot starts 16-byte aligned).
 * stats (optional, [n, 2*heads]): per row and head the softmax max and
 * denominator (sum + 1e-10), kept for kgx_gatv2_backward.
 * drop_key (optional): attention dropout (training, gatv2_conv.py:252-253):
 * alpha of (slot e, head h) is multiplied by the kgx_dropout_mask value of
 * (seed, drop_key[e], h); the denominator is not.
 * ------------------------------------------------------------------------- */
int kgx_gatv2(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
              const int32_t* items, int64_t n_items,
              const int32_t* split, int64_t n_split,
              const int32_t* col, const float* h_src, const float* h_dst, int64_t ld_h,
              const float* att, int heads, int channels, float negative_slope,
              float* out, int64_t ld_out, const float* bias,
              float* partials, float* stats,
              const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of kgx_gatv2 (autograd of GATv2Conv's propagate, gatv2_conv.py:
 * 241-352).  Needs the forward's output `out` (bias included when bias is
 * given) and its per-row softmax `stats` ([n, 2*heads]: max, denominator;
 * kgx_gatv2's optional last output).  Given G = d loss / d out, writes
 * d h_dst (destination CSR + its schedule; split rows via partials), d h_src
 * (pulled over the TRANSPOSED graph: t_rowptr/t_rows/t_items/t_split over
 * sources, t_col = destination row, t_slot = forward CSR slot of each
 * transposed slot), and ADDS d att (grad_att zeroed by the caller).
 * alpha_ws / ds_ws: E' * heads floats of workspace; partials:
 * max(n_slots, t_n_slots) * heads*channels floats.  The bias gradient is a
 * column sum the caller takes.
 * ------------------------------------------------------------------------- */
int kgx_gatv2_backward(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                       const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                       const int32_t* col, const float* h_src, const float* h_dst, int64_t ld_h,
                       const float* att, int heads, int channels, float negative_slope,
                       const float* out, int64_t ld_out, const float* bias, const float* stats,
                       const float* grad_out, int64_t ld_grad,
                       const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
                       const int32_t* t_items, int64_t t_n_items, const int32_t* t_split, int64_t t_n_split,
                       const int32_t* t_col, const int32_t* t_slot,
                       float* grad_h_src, float* grad_h_dst, int64_t ld_grad_h, float* grad_att,
                       float* alpha_ws, float* ds_ws, float* partials,
                       const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * kgx_gatv2 with edge features (PyG's GATv2Conv with edge_dim, on the shared-
 * weight layer): one projected edge row enters the score, and only the score.
 * For the row's CSR slots t (source j_t = col[t], edge row eps_t):
 *   z_t[c]  = (h_dst[i,h,c] + h_src[j_t,h,c]) + eps_t[h,c]
 *                                     (two rounded fp32 adds, in this order)
 *   s_t     = sum_c att[h,c] * leaky_relu(z_t[c], slope)
 *   alpha_t = exp(s_t - m) / (sum_t' exp(s_t' - m) + 1e-10)
 *   out[i,h,:] = sum_t alpha_t * mask_t * h_src[j_t,h,:]  (+ bias)
 * The message stays h_src[j_t] (kgx_dot_attention_edge adds eps there too).
 * e: the edge table [n_e, ld_e >= heads*channels], fp32, unit column stride.
 * e_idx: the edge row of each CSR slot ([kept] int32); NULL: the slot itself
 * (e is in CSR order).  A row outside [0, n_e) means the slot has no edge
 * feature: its eps is zeros.  Nothing is read out of range.  e == NULL (or
 * n_e == 0) is kgx_gatv2, which forwards here.  e joins the layout's alignment
 * inputs (16-byte pointer and ld_e a multiple of 4 for the float4 layouts).
 * Everything else -- schedule, partials, stats, dropout, bias -- is kgx_gatv2's.
 * Errors, before any device work: as kgx_gatv2; with e given, KGX_ERR_ARG for
 * ld_e < heads*channels, ld_e >= 2^31, and n_e outside [0, 2^31).
 * ------------------------------------------------------------------------- */
int kgx_gatv2_edge(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                   const int32_t* items, int64_t n_items,
                   const int32_t* split, int64_t n_split,
                   const int32_t* col, const float* h_src, const float* h_dst, int64_t ld_h,
                   const float* e, int64_t ld_e, int64_t n_e, const int32_t* e_idx,
                   const float* att, int heads, int channels, float negative_slope,
                   float* out, int64_t ld_out, const float* bias,
                   float* partials, float* stats,
                   const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of kgx_gatv2_edge.  As kgx_gatv2_backward with z_t formed by the
 * forward's two adds in both passes (so lrelu'(z_t) is taken at the forward's
 * z_t), and one more gradient, written by the destination pass:
 *   grad_e[eps_t][h,c] = ds_t * att[h,c] * lrelu'(z_t[c])      (lrelu'(0) = slope)
 * grad_e: [n_e, ld_ge >= heads*channels].  The destination pass stores the row
 * of every slot that has an edge row (chunks of a split row store their own
 * slots' rows; no partials): one writer per element when no two slots share an
 * edge row.  Rows of no kept slot are not written -- the caller zeroes them.
 * t_e_idx: the edge row of each TRANSPOSED slot (required with e; the source
 * pass gathers eps_t beside h_dst[i] and G_i).  e and grad_e join the layout's
 * alignment inputs.  alpha_ws / ds_ws / partials as kgx_gatv2_backward.
 * Errors, before any device work: as kgx_gatv2_backward; with e given,
 * KGX_ERR_ARG for grad_e or t_e_idx missing, ld_e or ld_ge < heads*channels or
 * >= 2^31, and n_e outside [0, 2^31).
 * ------------------------------------------------------------------------- */
int kgx_gatv2_edge_backward(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                            const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                            const int32_t* col, const float* h_src, const float* h_dst, int64_t ld_h,
                            const float* e, int64_t ld_e, int64_t n_e, const int32_t* e_idx,
                            const float* att, int heads, int channels, float negative_slope,
                            const float* out, int64_t ld_out, const float* bias, const float* stats,
                            const float* grad_out, int64_t ld_grad,
                            const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
                            const int32_t* t_items, int64_t t_n_items, const int32_t* t_split, int64_t t_n_split,
                            const int32_t* t_col, const int32_t* t_slot, const int32_t* t_e_idx,
                            float* grad_h_src, float* grad_h_dst, int64_t ld_grad_h, float* grad_att,
                            float* grad_e, int64_t ld_ge,
                            float* alpha_ws, float* ds_ws, float* partials,
                            const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused dot-product (query / key / value) graph attention: PyG's
 * TransformerConv message passing without edge features, in one pass with an
 * online segment softmax.  Destination row i, head h, edges e of the row
 * (source j_e = col[e]):
 *   s_e = scale * sum_c q[i,h,c] * k[j_e,h,c]
 *   m = max_e s_e,  l = sum_e exp(s_e - m)          (no epsilon)
 *   out[i,h,:] = sum_e exp(s_e - m) / l * mask_e * v[j_e,h,:]
 * mask_e = kgx_dropout_mask(seed, drop_key[e], h) when drop_key is given, else 1.
 * q: [n_dst, ld_q]; k, v: [n_src, ld_k], [n_src, ld_v]; fp32, unit column
 * stride, separate leading dimensions (k and v may be the two column halves of
 * one [n_src, 2*heads*channels] tensor).
 * Work list as kgx_gatv2: items == NULL reduces every row of `rows` whole, in
 * CSR order; otherwise split chunks write [H*C acc | H m | H l] to `partials`
 * (n_slots * ld_p floats, ld_p = heads*channels + 2*heads rounded up to a
 * multiple of 4) and a fix-up merges them in chunk order.
 * stats (optional, [n_dst, 2*heads]): (m, l), kept for the backward.
 * A row without edges is a zero row with stats (-inf, 0); a -inf score has
 * weight 0; a (row, head) whose scores are all -inf, or that contains +inf or
 * NaN, is NaN in its own block of `channels` columns only.  No atomics: a run
 * gives the same bits every time.
 * Errors, before any device work: KGX_ERR_UNSUPPORTED when heads *
 * next_pow2(ceil(channels / K)) > 64 for the widest usable K channels per lane
 * (8, 4 or 16 with 16-byte aligned pointers and leading dimensions that are
 * multiples of 4, else 2 or 1); KGX_ERR_ARG for null pointers, bad sizes,
 * ld < heads*channels, ld >= 2^31, drop_p outside [0, 1), and split rows
 * without a split list or partials.
 * ------------------------------------------------------------------------- */
int kgx_dot_attention(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                      const int32_t* items, int64_t n_items,
                      const int32_t* split, int64_t n_split,
                      const int32_t* col, const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                      const float* v, int64_t ld_v, int heads, int channels, float scale,
                      float* out, int64_t ld_out, float* partials, float* stats,
                      const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of kgx_dot_attention.  Needs the forward's `out` and `stats`.  With
 * G = d loss / d out, D[i,h] = <G[i,h,:], out[i,h,:]>, p_e = exp(s_e - m) / l
 * and ds_e = p_e * (mask_e * <G_i, v_j>_h - D[i,h]), two passes that both
 * recompute p_e from q, k and stats:
 *   destination pass (forward CSR + schedule): dsum_ws = D ([n_dst, heads]),
 *     grad_q[i] = scale * sum_e ds_e * k[j_e];
 *   source pass (transposed CSR + schedule; t_col = destination row, t_key =
 *     input edge id of each transposed slot, the dropout key):
 *     grad_v[j] = sum_e p_e * mask_e * G_i,  grad_k[j] = scale * sum_e ds_e * q_i.
 * Split rows go through per-chunk partials summed in chunk order; partials:
 * max(n_slots, t_n_slots) * 2*heads*channels floats.  No atomics and no
 * E x heads buffer.  Errors as the forward's.
 * ------------------------------------------------------------------------- */
int kgx_dot_attention_backward(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                               const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                               const int32_t* col, const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                               const float* v, int64_t ld_v, int heads, int channels, float scale,
                               const float* out, int64_t ld_out, const float* stats,
                               const float* grad_out, int64_t ld_grad,
                               const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
                               const int32_t* t_items, int64_t t_n_items, const int32_t* t_split, int64_t t_n_split,
                               const int32_t* t_col, const int32_t* t_key,
                               float* grad_q, int64_t ld_gq, float* grad_k, int64_t ld_gk,
                               float* grad_v, int64_t ld_gv, float* dsum_ws, float* partials,
                               const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * kgx_dot_attention with edge features (PyG's TransformerConv with edge_dim):
 * one projected edge row is added to the key in the score and to the value in
 * the message.  For the row's CSR slots t (source j_t = col[t], edge row eps_t):
 *   k'_t = k[j_t,h,:] + eps_t[h,:],  v'_t = v[j_t,h,:] + eps_t[h,:]
 *                                              (one rounded fp32 add per element)
 *   s_t = scale * sum_c q[i,h,c] * k'_t[c],  m, l as above (no epsilon)
 *   out[i,h,:] = sum_t exp(s_t - m) / l * mask_t * v'_t
 * e: the edge table [n_e, ld_e >= heads*channels], fp32, unit column stride.
 * e_idx: the edge row of each CSR slot ([kept] int32); NULL: the slot itself
 * (e is in CSR order).  A row outside [0, n_e) means the slot has no edge
 * feature: its eps is zeros (the self-loop slots of a KGX_CSR_SELF_LOOPS graph,
 * whose edge id is E + i, against a table of the E input edges).  Nothing is
 * read out of range.  e == NULL (or n_e == 0) is kgx_dot_attention, which
 * forwards here.  e joins the layout's alignment inputs (16-byte pointer and
 * ld_e a multiple of 4 for the float4 layouts).  Everything else -- schedule,
 * partials, stats, dropout, -inf / +inf / NaN per (row, head), empty rows, no
 * atomics -- is kgx_dot_attention's.
 * Errors, before any device work: as kgx_dot_attention (KGX_ERR_UNSUPPORTED
 * for the same shapes); with e given, KGX_ERR_ARG for ld_e < heads*channels,
 * ld_e >= 2^31, and n_e outside [0, 2^31).
 * ------------------------------------------------------------------------- */
int kgx_dot_attention_edge(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                           const int32_t* items, int64_t n_items,
                           const int32_t* split, int64_t n_split,
                           const int32_t* col, const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                           const float* v, int64_t ld_v,
                           const float* e, int64_t ld_e, int64_t n_e, const int32_t* e_idx,
                           int heads, int channels, float scale,
                           float* out, int64_t ld_out, float* partials, float* stats,
                           const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of kgx_dot_attention_edge.  As kgx_dot_attention_backward with k'
 * and v' in the place of k[j] and v[j] (all three kernels form them by the
 * same add, so s_t has the forward's bits), ds_t = p_t * (mask_t * <G_i,
 * v'_t>_h - D[i,h]), and a fourth gradient:
 *   grad_q[i]     = scale * sum_t ds_t * k'_t                 destination pass
 *   grad_k[j], grad_v[j] as without edge features                  source pass
 *   grad_e[eps_t] = scale * ds_t * q_i + p_t * mask_t * G_i   destination pass
 * grad_e: [n_e, ld_ge >= heads*channels].  The destination pass stores the row
 * of every slot that has an edge row (chunks of a split row store their own
 * edges' rows; no partials): one writer per element when no two slots share an
 * edge row.  Rows of no kept slot are not written -- the caller zeroes grad_e
 * when the graph dropped input edges.  t_e_idx: the edge row of each
 * TRANSPOSED slot (required with e; the source pass gathers eps_t beside q_i
 * and G_i).  e and grad_e join the layout's alignment inputs.
 * Errors, before any device work: as kgx_dot_attention_backward; with e given,
 * KGX_ERR_ARG for grad_e or t_e_idx missing, ld_e or ld_ge < heads*channels or
 * >= 2^31, and n_e outside [0, 2^31).
 * ------------------------------------------------------------------------- */
int kgx_dot_attention_edge_backward(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                                    const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                                    const int32_t* col, const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                                    const float* v, int64_t ld_v,
                                    const float* e, int64_t ld_e, int64_t n_e, const int32_t* e_idx,
                                    int heads, int channels, float scale,
                                    const float* out, int64_t ld_out, const float* stats,
                                    const float* grad_out, int64_t ld_grad,
                                    const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
                                    const int32_t* t_items, int64_t t_n_items,
                                    const int32_t* t_split, int64_t t_n_split,
                                    const int32_t* t_col, const int32_t* t_key, const int32_t* t_e_idx,
                                    float* grad_q, int64_t ld_gq, float* grad_k, int64_t ld_gk,
                                    float* grad_v, int64_t ld_gv, float* grad_e, int64_t ld_ge,
                                    float* dsum_ws, float* partials,
                                    const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused segment softmax + weighted sum, the attention readouts' pooling (one
 * pass over x, online softmax; plus a fix-up for split segments):
 *   out[g,:] = sum_{i in g} softmax_g(s)_i * x[i,:]
 *   softmax_g(s)_i = exp(s_i - m_g) / l_g,  m_g = max_{i in g} s_i,
 *   l_g = sum_{i in g} exp(s_i - m_g)        (no epsilon in the denominator)
 * Replaces ops.softmax(scores, axis=0) and ops.sum(weights * inputs, axis=0)
 * of AttentionPooling (pooling/attention_pooling.py:409-412) and of every
 * Set2Set processing step (:175-180, :206-211), per graph of a batch.
 * Segments: a CSR rowptr[n_seg+1] over segment slots, `rows` (every segment,
 * any order) and optionally the schedule items / split of kgx_schedule_build;
 * with items == NULL each row of `rows` is reduced whole by one lane group.
 * idx[slot] = node of a slot (a segment CSR's col), NULL = identity (sorted
 * batches, the single graph rowptr = {0, N}).  x: [N, ld_x >= F], unit column
 * stride.  Exactly one score source:
 *   s [N]                      scores given, or
 *   score_u [F], score_c [n_seg]   s_i = act(x_i . score_u + score_c[g]), act =
 *     tanh with KGX_POOL_SCORE_TANH else identity, computed from the row just
 *     loaded and stored to s_out [N] (Set2Set's Dense(1, tanh) over
 *     concat(x, h): :165-172, with score_c[g] = h_g . k_h + b).
 * Outputs: out [n_seg, ld_out >= F]; stats (optional) [n_seg, 2] = (m, l),
 * kept for kgx_softmax_pool_backward.  partials: n_slots * (F + 2) floats when
 * rows are split (per slot [F acc | m | l], merged in chunk order).
 * A -inf score has weight 0; an empty segment is a zero row (the sum over no
 * rows); a segment whose scores are all -inf, or that holds +inf or NaN, is
 * NaN in its own row only (torch.softmax).  Numerator and denominator are
 * accumulated in fp64; no atomics: the same bits on every run.
 * F: 1 .. KGX_POOL_MAX_F (float4 lanes when F % 4 == 0 and x, out, score_u
 * rows are 16-byte aligned, scalar lanes otherwise).
 * Errors, before any device call: KGX_ERR_ARG for bad sizes, null pointers,
 * both or neither score source, ld < F, split rows without split list and
 * partials; KGX_ERR_UNSUPPORTED for F > KGX_POOL_MAX_F.
 * ------------------------------------------------------------------------- */
enum { KGX_POOL_SCORE_TANH = 1 };
enum { KGX_POOL_MAX_F = 256 };
int kgx_softmax_pool(const int32_t* rowptr, const int32_t* rows, int64_t n_seg,
                     const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                     const int32_t* idx, const float* x, int64_t ld_x, int64_t F,
                     const float* s, const float* score_u, const float* score_c, int flags, float* s_out,
                     float* out, int64_t ld_out, float* stats, float* partials, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Backward of kgx_softmax_pool (autograd of the softmax / weighted sum of
 * attention_pooling.py:175-180, :409-412).  Given G = d loss / d out [n_seg,
 * ld_grad], the forward's out, stats and scores s (given, or its s_out):
 *   alpha_i     = exp(s_i - m_g) / l_g
 *   grad_x[i,:] = alpha_i * G[g,:]                       [N, ld_grad_x >= F]
 *   grad_s[i]   = alpha_i * (x_i . G_g - out_g . G_g)    [N]
 * in one pass over x.  seg [N]: the segment of every node, NULL = all nodes in
 * segment 0; ids outside [0, n_seg) get zero gradient.  No schedule, partials
 * or atomics.  grad_x is the pooled sum's part only: a fused score's chain
 * (d tanh, score_u, score_c) is the caller's, from grad_s.
 * Errors as kgx_softmax_pool: null pointers and ld < F are KGX_ERR_ARG,
 * F > KGX_POOL_MAX_F is KGX_ERR_UNSUPPORTED, before any device call.
 * ------------------------------------------------------------------------- */
int kgx_softmax_pool_backward(int64_t N, int64_t n_seg, const int32_t* seg,
                              const float* x, int64_t ld_x, int64_t F,
                              const float* s, const float* stats, const float* out, int64_t ld_out,
                              const float* grad_out, int64_t ld_grad,
                              float* grad_x, int64_t ld_grad_x, float* grad_s, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Dense node transform (the layers' keras Dense / ops.matmul), one launch:
 *   out[i,:] (+)= ACT( bias + x0[i,:K0] @ W0 + x1[i,:K1] @ W1 )
 * Replaces GINConv's MLP Dense (gin_conv.py:129-162, applied at :225),
 * SAGEConv's lin_self(x) + lin_neigh(aggr) + bias (sage_conv.py:407-428: both
 * terms in ONE pass), GATv2Conv's shared linear map (gatv2_conv.py:224-239) and
 * GCNConv's x @ kernel (gcn_conv.py:233-235) where the fused kernel does not
 * apply.  f32-accurate: the product runs on bf16 MFMA as the six significant
 * cross products of a three-way bf16 split of both operands (dropped terms
 * <= 2^-24 |x w|); tolerance-equal to fp32 GEMM, not bit-equal.
 * Shapes: K0 + K1 <= KGX_DENSE_MAX_K, N <= KGX_DENSE_MAX_N, K0 and K1
 * multiples of 4, x rows 16-byte aligned with ld % 4 == 0; W0 [K0, N] and
 * W1 [K1, N] row-major contiguous; x1/W1 may be NULL with K1 = 0; bias [N] or
 * NULL.  KGX_DENSE_RELU: out = max(., 0) (Dense(activation='relu'));
 * KGX_DENSE_ACCUMULATE: out += (before RELU).
 * ------------------------------------------------------------------------- */
enum { KGX_DENSE_RELU = 1, KGX_DENSE_ACCUMULATE = 2 };
enum { KGX_DENSE_MAX_K = 256, KGX_DENSE_MAX_N = 256 };
int kgx_dense(int64_t M, const float* x0, int64_t ld_x0, int64_t K0, const float* W0,
              const float* x1, int64_t ld_x1, int64_t K1, const float* W1, int64_t N,
              const float* bias, int flags, float* out, int64_t ld_out, kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Row gather out[i,:] = table[rows[i], :] — packs halo rows for the multi-GPU
 * exchange (no reference counterpart; the reference is single-device) and
 * scatters per-edge values back to input edge order.
 * ------------------------------------------------------------------------- */
int kgx_gather_rows(const float* table, int64_t ld_table, const int32_t* rows,
                    int64_t n, int64_t F, float* out, int64_t ld_out,
                    kgx_stream_t stream);
/* out[perm[i]] = in[i] for i < n (int32 perm) — CSR-order -> input-order. */
int kgx_scatter_f32(const float* in, const int32_t* perm, int64_t n, float* out,
                    kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Synthetic R-MAT edge generator (bench/test input; the reference has no
 * generator — its perf tests use numpy.random, tests/performance/
 * test_large_graphs.py:86-110).  Counter-based and bit-reproducible: edge k of
 * (seed, scale, a, b, c) is the same on every device and in the numpy
 * restatement (oracle/rmat.py).  Probabilities are 24-bit fixed point
 * (p * 2^24).  Raw ids (mod n_nodes) are relabelled by a keyed Feistel
 * permutation.  Writes edges [e_begin, e_begin + e_count).
 * ------------------------------------------------------------------------- */
int kgx_rmat_edges(uint64_t seed, int scale, int64_t n_nodes,
                   uint32_t a24, uint32_t b24, uint32_t c24,
                   int64_t e_begin, int64_t e_count,
                   int32_t* src, int32_t* dst, kgx_stream_t stream);

/* Keep edges whose dst lies in [lo, hi): stream compaction used to carve one
 * rank's destination-range shard out of a generated batch.  n_out (host)
 * receives the count; out arrays need capacity n.  Syncs once.               */
int kgx_select_dst_range(const int32_t* src, const int32_t* dst, int64_t n,
                         int64_t lo, int64_t hi, int32_t* src_out, int32_t* dst_out,
                         void* workspace, size_t workspace_bytes, int64_t* n_out,
                         kgx_stream_t stream);
int kgx_select_workspace_bytes(int64_t n, size_t* bytes);

/* ---------------------------------------------------------------------------
 * Neighbour sampling for mini-batch GraphSAGE training (no reference
 * counterpart: the reference trains full-batch; the semantics are those of
 * PyG's NeighborLoader without replacement).
 *
 * kgx_sample_neighbors: one hop of fan-out sampling over a destination CSR
 * (rowptr[n_rows+1], col, eid of kgx_csr_build).  Row i of the result belongs
 * to seeds[i] (int32 row ids) and holds min(deg(seeds[i]), fanout) edges;
 * fanout = -1 takes every neighbour.
 *   out_rowptr[n_seeds+1]  offsets of the rows (a count kernel + exclusive scan)
 *   out_src[cap]           global source id of each sampled edge
 *   out_eid[cap]           input edge id of each sampled edge (to carry edge
 *                          weights or attributes along)
 * cap >= n_seeds * fanout; with fanout = -1 cap must cover the seeds' total
 * degree (else KGX_ERR_ARG after the sync, and out_src / out_eid are not
 * written).  A row of degree d <= fanout (or fanout = -1) is taken whole, in
 * CSR order.  A row of degree d > fanout = k takes the k distinct CSR slots
 * pi(0), ..., pi(k-1), emitted in that order, pi(t) = (phi(t) + rot) mod d,
 * phi = a 4-round Feistel permutation of [0, 2^(2 hb)), hb =
 * ceil(ceil_log2(d) / 2) bits per half (a superset smaller than 4 d),
 * cycle-walked into [0, d):
 *   round i:  (L, R) <- (R, L ^ (splitmix64(key[i] ^ R) & (2^hb - 1))),
 *   x = (L << hb) | R, repeated while the result is >= d.
 * The keys and the rotation depend on (seed, hop, the row's global id) only
 * (uint64 arithmetic modulo 2^64, splitmix64 as in kgx_rmat_edges):
 *   hs     = splitmix64(seed ^ splitmix64(uint64(uint32(hop))))
 *   rs     = splitmix64(hs ^ uint64(row))
 *   key[i] = splitmix64(rs + i),  i = 0..3
 *   rot    = ((splitmix64(rs + 4) >> 32) * d) >> 32          (in [0, d))
 * (the rotation makes every slot of a row equally likely: four Feistel rounds
 * on halves of one or two bits are biased even under ideal keys),
 * so a node's sample is independent of the batch it appears in, of its
 * position in `seeds`, of the grid size and of the device; one lane computes
 * each output slot and no atomic decides an output value (tests/sampling_ref.py
 * restates it in numpy, bit for bit).  Sampling is over CSR slots: an edge the
 * input lists twice has two slots and can be drawn once per copy.
 * info[4] (host): sampled edges (= out_rowptr[n_seeds]), seeds out of range,
 * 0, 0.  Synchronises `stream` once, like kgx_csr_build.
 * Errors before any device call (KGX_ERR_ARG): null pointers, fanout == 0 or
 * < -1, n_seeds < 0, n_seeds * fanout >= 2^31, cap < n_seeds * fanout, a
 * workspace smaller than kgx_sample_workspace_bytes(n_seeds).  n_seeds == 0:
 * KGX_OK, nothing launched.  A seed outside [0, n_rows) is counted on the
 * device and reported as KGX_ERR_INDEX after the sync (its row is empty and
 * nothing is read for it).
 *
 * kgx_relabel_frontier: compacts one hop into local ids.
 *   nodes[n_known]      the node list so far (global ids, seeds first, distinct)
 *   frontier[n_f]       the rows just expanded: frontier[i] is row i of
 *                       out_rowptr (hop 0: the seeds); every entry is in nodes
 *   out_rowptr, out_src the hop's result, n_edges = out_rowptr[n_f]
 *   map[n_nodes]        caller-owned int32 scratch: every entry -1 on entry,
 *                       and -1 again on return (also on the errors below)
 * Outputs:
 *   new_nodes[n_edges]  (capacity) the sampled sources not in nodes, each once,
 *                       in ascending global id (radix sort, adjacent-unique
 *                       flags, scan, select); local id = n_known + rank
 *   src_local[n_edges]  local id of out_src[e]
 *   dst_local[n_edges]  local id of the frontier row edge e belongs to
 * The map is written for nodes at the start (map[nodes[i]] = i) and reset for
 * nodes and new_nodes at the end: the work is O(n_known + n_edges), never
 * O(n_nodes).  info[4] (host): new nodes, duplicate entries of nodes, ids out
 * of range, 0.  Synchronises `stream` once.  Duplicate ids in nodes are found
 * on the device (every entry re-reads the map after all have written it) and
 * reported as KGX_ERR_ARG after the sync; an id outside [0, n_nodes) in nodes,
 * frontier or out_src as KGX_ERR_INDEX (it is never used as an index).
 * Errors before any device call (KGX_ERR_ARG): null pointers, negative sizes,
 * n_known + n_edges >= 2^31, edges without a frontier row, a workspace smaller
 * than kgx_relabel_workspace_bytes(n_edges, n_nodes).
 * ------------------------------------------------------------------------- */
int kgx_sample_workspace_bytes(int64_t n_seeds, size_t* bytes);
int kgx_sample_neighbors(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t n_rows,
                         const int32_t* seeds, int64_t n_seeds, int fanout, uint64_t seed, int hop,
                         int32_t* out_rowptr, int32_t* out_src, int32_t* out_eid, int64_t cap,
                         void* workspace, size_t workspace_bytes, int64_t* info, kgx_stream_t stream);
int kgx_relabel_workspace_bytes(int64_t n_edges, int64_t n_nodes, size_t* bytes);
int kgx_relabel_frontier(const int32_t* nodes, int64_t n_known, const int32_t* frontier, int64_t n_f,
                         const int32_t* out_rowptr, const int32_t* out_src, int64_t n_edges,
                         int32_t* map, int64_t n_nodes, int32_t* new_nodes, int32_t* src_local,
                         int32_t* dst_local, void* workspace, size_t workspace_bytes, int64_t* info,
                         kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Sampled blocks: the CSR pair of one bipartite layer graph of a mini-batch
 * (DGL's "block" / message-flow graph, PyG's trim_to_layer).
 *
 * The sampler gives local ids to the seeds first, then hop by hop, and emits
 * the hops' edges in that order.  With P_h = the number of nodes after hop
 * h - 1 (P_0 = the seeds): the merged dst array is non-decreasing, the edges
 * of hops 0..h are a prefix of the edge list, their destinations are < P_h and
 * their sources < P_{h+1}.  So the edge list is a destination CSR as it
 * stands (col = src, eid = the edge's position), the graph a layer needs is a
 * prefix of it, and only rowptr / deg and the transposed CSR are computed.
 *
 * kgx_block_csr: src[E], dst[E] device int32, dst non-decreasing, src in
 * [0, n_src), dst in [0, n_dst) (no wrap of negative ids: these are the
 * sampler's local ids).
 *   rowptr[n_dst+1], deg[n_dst]   optional (both NULL to skip): offsets of the
 *                                 destination rows, by binary search of dst
 *   t_rowptr[n_src+1], t_deg[n_src]
 *   t_col[E]                      destination of each edge, source-major
 *   t_eid[E]                      position of each edge in src / dst, ascending
 *                                 inside every row: the input-edge order of
 *                                 graph.transpose, and the edge's forward slot
 * The transposed side is a stable rocprim radix sort of (src, position) over
 * ceil_log2(n_src) bits and a binary search of the sorted keys; the work is
 * O(E + (n_src + n_dst) log E).  Every output is a pure function of the
 * inputs: atomics only count violations and fold the two maxima.
 * info[4] (host): max in-degree, max out-degree, edges with dst[e] < dst[e-1],
 * ids out of range.  Synchronises `stream` once.  Order violations:
 * KGX_ERR_ARG; ids out of range: KGX_ERR_INDEX (reported first when both
 * occur); in either case none of the output arrays is written.
 * Errors before any device call (KGX_ERR_ARG): null pointers, negative sizes,
 * E >= 2^31, a workspace smaller than kgx_block_workspace_bytes(E, n_src).
 * E == 0, n_dst == 0, n_src != n_dst and rows of degree 0 are all valid.
 * ------------------------------------------------------------------------- */
int kgx_block_workspace_bytes(int64_t E, int64_t n_src, size_t* bytes);
int kgx_block_csr(const int32_t* src, const int32_t* dst, int64_t E, int64_t n_src, int64_t n_dst,
                  int32_t* rowptr, int32_t* deg, int32_t* t_rowptr, int32_t* t_deg, int32_t* t_col,
                  int32_t* t_eid, void* workspace, size_t workspace_bytes, int64_t* info,
                  kgx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Link prediction: edge scores from node rows (the SDDMM-shaped counterpart of
 * kgx_spmm) and the negative sampler that feeds it.  No reference counterpart.
 *
 * kgx_edge_dot:
 *   out[p * ld_out + k] = sum_f xa[a_idx[p], f] * xb[b_idx[p * K + k], f]    p < P, k < K
 * xa [n_a, ld_a >= F] and xb [n_b, ld_b >= F] are fp32 with unit column stride
 * and may be the same pointer; a_idx[P] and b_idx[P * K] are int32.  K = 1 is a
 * plain pair list, K = 1 + Q one positive followed by its Q negatives: the xa
 * row is loaded once per p, so a positive costs (1 + K) * 4F bytes.
 *   perm   optional int32[P], a permutation of [0, P): row p is stored at
 *          out[perm[p] * ld_out + k] (a graph's own edges scored in CSR order
 *          and returned in input-edge order).  An entry outside [0, P) is
 *          counted in `bad` and its row is not stored.
 *   bad    optional device int32, zeroed by the caller, never read back here:
 *          the number of indices outside their table.  Such an index is clamped
 *          for the load and its score is stored as NaN; nothing is read out of
 *          range.
 * Every score is a function of its two rows and F alone: with V = 4, 2 or 1
 * the widest of those dividing F and G = min(64, next_pow2(F / V)), lane l of a
 * group of G lanes adds the products of columns (t * G + l) * V .. + V, t = 0,
 * 1, ..., in column order into one accumulator (separately rounded multiply and
 * add, starting from +0), and the G accumulators are folded by the xor
 * butterfly of distances G/2, ..., 1.  Rows that are not 16 (8) byte aligned
 * are read with narrower loads in the same lane layout, so alignment, p, k, K,
 * P, perm and the grid size never change a bit; inf and NaN follow IEEE in
 * their own pair's score only.  No allocation, no synchronise.
 * Errors before any device call (KGX_ERR_ARG): null a_idx / b_idx / out (xa /
 * xb unless F == 0), negative sizes, K < 1, ld_a < F, ld_b < F, ld_out < K, P * K >= 2^31,
 * an ld >= 2^31, an empty table with P > 0.  P == 0: KGX_OK, nothing launched;
 * F == 0: every score is +0.
 *
 * kgx_negative_edges: Q corrupted sources for each positive (source ->
 * destination a[p]) over a destination CSR whose rows are sorted ascending
 * (col_sorted).  One lane per output; all arithmetic uint64 modulo 2^64,
 * splitmix64 as in kgx_sample_neighbors:
 *   ks   = splitmix64(seed ^ splitmix64(uint64(uint32(keys[p]))))
 *   rs   = splitmix64(ks + q)                                q < Q
 *   try t = 0 .. max_tries-1:  r = splitmix64(rs + t);  cand = ((r >> 32) * n_src) >> 32
 *   reject cand if (flags & KGX_NEG_NO_SELF) and cand == a[p], or
 *                  (flags & KGX_NEG_REJECT_EDGES) and cand is in
 *                  col_sorted[rowptr[a[p]] .. rowptr[a[p] + 1])  (binary search)
 *   out[p * ld_out + q] = the first candidate not rejected
 * If every try is rejected the output is the last try's candidate and stats[0]
 * counts it.  An a[p] outside [0, n_dst) is counted in stats[1] (once per p);
 * nothing is read for it and its outputs are -1.  stats: device int32[2],
 * zeroed by the caller; no output value depends on an atomic.  With keys = the
 * positives' input edge ids a positive draws the same negatives in every
 * batch, at every position, on every device (tests/negative_ref.py restates it
 * bit for bit).  ld_out >= Q: `out` may point into column 1 of a [P, 1 + Q]
 * index array.  No synchronise.
 * Errors before any device call (KGX_ERR_ARG): null a / keys / out / stats
 * (rowptr / col_sorted with KGX_NEG_REJECT_EDGES), Q < 1, max_tries outside
 * 1..64, n_src < 1 or >= 2^31, negative sizes, unknown flags, ld_out < Q,
 * P * Q >= 2^31.  P == 0: KGX_OK.
 * ------------------------------------------------------------------------- */
enum { KGX_NEG_NO_SELF = 1, KGX_NEG_REJECT_EDGES = 2 };
enum { KGX_EDGE_DOT_U = 8 }; /* candidate rows in flight per group */
int kgx_edge_dot(const float* xa, int64_t n_a, int64_t ld_a, const float* xb, int64_t n_b, int64_t ld_b,
                 int64_t F, const int32_t* a_idx, const int32_t* b_idx, int64_t P, int64_t K,
                 const int32_t* perm, float* out, int64_t ld_out, int32_t* bad, kgx_stream_t stream);
int kgx_negative_edges(const int32_t* rowptr, const int32_t* col_sorted, int64_t n_dst, int64_t n_src,
                       const int32_t* a, const int32_t* keys, int64_t P, int Q, uint64_t seed, int max_tries,
                       int flags, int32_t* out, int64_t ld_out, int32_t* stats, kgx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KGX_H_ */
