/*
 * tnco_hip.h -- C ABI of libtnco_hip.so: batched simulated annealing of
 * tensor-network contraction trees on one MI355X (gfx950).
 *
 * Drop-in boundary.  Each entry point names the reference interface it replaces
 * (paths relative to the google-research/tnco checkout).  The reference exposes
 * ONE replica per pybind11 object and is stepped from Python
 * (tnco/app/infinite_memory/sa.py:199-209); this ABI carries MANY replicas per
 * handle and a whole beta schedule per call.  Plain pointers and sizes only;
 * every input is copied at create time and every output is copied into
 * caller-owned buffers (the reference takes its ctree by value and clones the
 * cost model, include/tnco/optimize/infinite_memory/optimizer.hpp:61-67).
 *
 * Threading: a handle is bound to one device and one stream and is not
 * thread-safe; distinct handles are independent.
 *
 * Status codes: 0 ok; TNCO_HIP_EINVAL -> ValueError in the Python shim
 * (std::invalid_argument / std::domain_error in the reference,
 * include/tnco/ctree.hpp:48-50, infinite_memory/optimizer.hpp:77-87);
 * TNCO_HIP_ERUNTIME -> RuntimeError; TNCO_HIP_ENOTIMPL -> NotImplementedError.
 * tnco_hip_last_error() returns the message of the last failing call on the
 * calling thread.
 *
 * Three families of entry points:
 *   the operator   tnco_hip_create / _run / _run_fw / _sync / _get_* / _set_* / _validate / _best / _destroy ...:
 *                  what the reference's Optimizer_<cost>[_<width>] objects do, batched;
 *   helpers        tnco_hip_random_trees / _greedy_trees[_device] / _linear_paths* (the host code either side of the
 *                  path), tnco_hip_comm_* (the one collective of a multi-GPU launch), device queries;
 *   diagnostics    tnco_hip_diag_*: counters, timers and internals the tests, bench.py and tools/ read.  They have
 *                  no reference counterpart and are NOT part of the drop-in contract (a binding of the reference
 *                  needs none of them; INTEGRATION.md's stub uses none).
 */
#ifndef TNCO_HIP_H_
#define TNCO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNCO_HIP_OK 0
#define TNCO_HIP_EINVAL 1
#define TNCO_HIP_ERUNTIME 2
#define TNCO_HIP_ENOTIMPL 3

/* Acceptance rule, include/tnco/optimize/prob/{base,greedy,mh}.hpp. */
#define TNCO_HIP_PROB_BASE 0
#define TNCO_HIP_PROB_GREEDY 1
#define TNCO_HIP_PROB_MH 2

/* cost_type / width_type, include/tnco/globals.hpp:81-117 (float64 / float32
 * only; long double and float1024 are CPU-only in the reference). */
#define TNCO_HIP_F64 0
#define TNCO_HIP_F32 1

typedef struct tnco_hip_ctx* tnco_hip_handle;

/*
 * Problem description = the arguments of
 *   tnco_core.ContractionTree(nodes, inds, dims, check_shared_inds)
 *     (include/tnco/ctree.hpp:59-94),
 *   SimpleCostModel / SimpleSparseIndsCostModel
 *     (include/tnco/optimize/infinite_memory/cost_model/simple.hpp:57-88,
 *      simple_sparse_inds.hpp:51-93), and
 *   Optimizer_<cost>(ctree, cmodel, seed=, disable_shared_inds=)
 *     (include/tnco/optimize/infinite_memory/optimizer.hpp:61-88,
 *      include/tnco/optimize/optimizer.hpp:57-82)
 * for n_replicas replicas at once.  N = 2*n_leaves-1, W = ceil(n_inds/64)
 * (at least 1); bit p of word p/64 of a mask <-> index position p.
 */
typedef struct tnco_hip_desc {
  int32_t n_leaves;            /* leaves occupy node slots [0, n_leaves), root is slot N-1 */
  int32_t n_inds;
  int64_t n_replicas;
  const uint64_t* leaf_masks;  /* [n_leaves][W]; identical for every replica */
  const uint64_t* output_mask; /* [W] legs of the result tensor, or NULL (none) */
  const int32_t* links;        /* per replica [3][N]: left[N], right[N], parent[N]; null = -1.  Host memory,
                                  or device memory of `device` (tnco_hip_greedy_trees_device) */
  int64_t links_stride;        /* int32 elements between replicas; 0 = one tree shared by all */
  const uint64_t* node_masks;  /* optional per replica [N][W] legs of EVERY node (the reference
                                  passes them in); NULL = derive them on the device from the
                                  leaves (rule of tnco/ctree.py:163-189) */
  int64_t node_masks_stride;   /* uint64 elements between replicas; 0 = shared */
  uint64_t dim_uniform;        /* used when dims == NULL */
  const uint64_t* dims;        /* [n_inds] or NULL; all-equal collapses to uniform (ctree.hpp:79-89) */
  const uint64_t* sparse_mask; /* [W] or NULL -> SimpleCostModel */
  uint64_t n_projs;            /* > 0 when sparse_mask != NULL */
  int32_t cost_dtype;          /* TNCO_HIP_F64 | TNCO_HIP_F32 */
  int32_t disable_shared_inds;
  const uint32_t* seeds;       /* [n_replicas] std::mt19937 seeds (already reduced mod 2^32) */
  int32_t device;              /* HIP device ordinal */
  int32_t width_dtype;         /* TNCO_HIP_F32 (the reference's default width_type) | TNCO_HIP_F64 */
  /* Finite width (include/tnco/optimize/finite_width/greedy/optimizer.hpp:72-115 and
   * finite_width/cost_model/simple.hpp:89-95): active when max_width is finite and >= 0; pass
   * NAN / INFINITY for the infinite-memory optimizer. */
  double max_width;
  uint64_t max_number_new_slices; /* finite_width/greedy/optimizer.hpp:226-321 (the reference's app
                                     always passes 0; any value is implemented) */
  const uint64_t* skip_slices;    /* [W] or NULL */
  const uint64_t* slices;         /* [W] per row: the `slices` constructor argument (no initial slicing, no
                                     PRNG draw), or NULL = greedy initial slicing (draws from the PRNG) */
  /* Restoring a batch -- the remaining constructor arguments, which Optimizer.__reduce__ round-trips
   * (tnco/optimize/infinite_memory/optimizer.py:243-245, finite_width/optimizer.py:343-346;
   * include/tnco/optimize/optimizer.hpp:57-77, infinite_memory/optimizer.hpp:61-88,
   * finite_width/greedy/optimizer.hpp:72-115).  As in the reference the caches are rebuilt from the
   * trees and min_total_cost = get_cost(min_ctree[, min_slices]).  All optional (zero / NULL). */
  const int32_t* min_links;       /* per replica [3][N] like `links`: min_ctree.  NULL = the current tree.  Host memory */
  int64_t min_links_stride;       /* int32 elements between replicas; 0 = one tree shared by all */
  const uint64_t* min_slices;     /* [W] per row: min_slices.  NULL = slices */
  int64_t slices_stride;          /* uint64 elements between the replicas' rows of `slices` and of `min_slices`;
                                     0 = one row shared by all */
  const uint32_t* prng_states;    /* [n_replicas][625]: prng_state of every replica (624 words + position, the
                                     numbers of the reference's string seed, optimize/optimizer.hpp:68-71);
                                     replaces `seeds`, which may then be NULL */
} tnco_hip_desc;

/* Replaces the Optimizer_<cost> constructor for a batch: copies inputs, builds
 * CostCache / HyperCache (include/tnco/optimize/infinite_memory/utils.hpp:22-116)
 * and validates every tree (ctree.hpp:101-152).  EINVAL with "Contraction is
 * not valid." / "Precision is too low." as the reference throws. */
int tnco_hip_create(const tnco_hip_desc* desc, tnco_hip_handle* out);

/* Diagnostics: the tree check of tnco_hip_create on EVERY one of `ntrees` trees ([3][N] each, `stride` >= 3N int32
 * apart, HOST memory), one code per tree into status_out (host): 0 valid, 1..6 the first failing check of
 * Tree::is_valid read strictly ("Nodes are not valid", "Last node should be root.", "There should be only one root.",
 * "All leaves should be first.", "Number of nodes is not constenst with the number of leaves.", "Tree is not valid."),
 * 7 = not every node is reached from the root ("Tree is not valid." too; the reference has no such check).
 * where = 0: the host check (what `links` / `min_links` in host memory get), no device use.  where = 1: the trees are
 * uploaded to `device` and checked by the kernel that device links get; it has no check 7 and answers 0 there. */
int tnco_hip_diag_tree_check(int32_t device, int32_t N, const int32_t* links, int64_t stride, int64_t ntrees, int where,
                             int32_t* status_out);

/* Replaces the Python step loop `for beta in betas: prob.beta = beta;
 * opt.update(prob)` (tnco/app/infinite_memory/sa.py:199-209 over
 * Optimizer::update, infinite_memory/optimizer.hpp:90-221): n_steps sweeps on
 * every replica, sweep k using betas[k].  The call copies `betas`, enqueues its
 * kernels and returns without waiting -- neither for them nor for the previous
 * call's (calls queue up on the device); any getter synchronises.  A handle whose
 * replicas do not fill whole rounds of resident workgroups runs every step as two
 * concurrent launches over half of the replicas each (streams of its own, forked
 * from / joined into the handle's stream): same results, no idle tail. */
int tnco_hip_run(tnco_hip_handle h, int prob_kind, const double* betas, int64_t n_steps);

/* Finite-width twin: `opt.update(prob, update_slices=(n % update_slices_every == 0))` for
 * n = step_offset, step_offset + 1, ... (tnco/app/finite_width/sa.py:219-233 over
 * finite_width/greedy/optimizer.hpp:117-390).  update_slices_every <= 0: never re-slice. */
int tnco_hip_run_fw(tnco_hip_handle h, int prob_kind, const double* betas, int64_t n_steps,
                    int64_t update_slices_every, int64_t step_offset);

/* slices / min_slices properties (finite_width/greedy/optimizer.hpp:66-67) of one replica, [W]
 * words each; either may be NULL. */
int tnco_hip_get_slices(tnco_hip_handle h, int64_t replica, uint64_t* slices, uint64_t* min_slices);

/* The same for k replicas at once: slices / min_slices [k][W] (either may be NULL). */
int tnco_hip_get_slices_many(tnco_hip_handle h, int64_t k, const int64_t* replicas, uint64_t* slices,
                             uint64_t* min_slices);

/* Diagnostics of the LAST re-slice of every replica (no reference counterpart; tests pick the replicas whose
 * re-slice took a rare path and compare exactly those with the oracle): how[r] = 1 the cost cache was re-priced
 * (fw_wave_kernel), 0 it was rebuilt in full (or the replica has no slices); n_changed[r] = indices
 * by which the proposed slices differed from the current ones (-1: not recorded -- the single-kernel form, or more
 * than the re-pricing handles).  Either may be NULL.  EINVAL for a handle without re-pricing. */
int tnco_hip_diag_reslice_info(tnco_hip_handle h, int32_t* how, int32_t* n_changed);

/* Diagnostics (no reference counterpart): what the re-slices of this handle did since it was created, in replica
 * re-slices (one replica at the end of one re-slicing sweep, greedy/optimizer.hpp:359-376).  out8[0] launched in
 * the re-priced form (one wavefront per replica); out8[1] of those, left to the full rebuild; why: out8[2] more
 * too-wide tensors / a deeper tree / more candidate legs than the wavefront form lists, out8[3] more changed indices
 * than it re-prices or an index it cannot place, out8[4] a cost outside a double's powers of two; out8[5] launched
 * in the walk + full-rebuild form; out8[6..7] reserved (0).  bench.py reports out8[1] / out8[0]. */
int tnco_hip_diag_fw_stats(tnco_hip_handle h, int64_t* out8);

int tnco_hip_sync(tnco_hip_handle h);

/* total_cost / min_total_cost properties (optimizer.hpp:253-257) of every
 * replica as raw doubles (the reference prints them to a 6-digit Decimal,
 * optimizer.hpp:278-289; callers wanting that format it host-side).
 * Either pointer may be NULL. */
int tnco_hip_get_costs(tnco_hip_handle h, double* total_cost, double* min_total_cost);

/* ctree / min_ctree read-only properties (optimize/optimizer.hpp:207-208) of
 * one replica.  which: 0 current, 1 best-so-far.  masks ([N][W]) may be NULL. */
int tnco_hip_get_tree(tnco_hip_handle h, int64_t replica, int which, int32_t* left,
                      int32_t* right, int32_t* parent, uint64_t* masks);

/* CostCache / HyperCache contents of one replica (what is_valid() rebuilds and
 * compares, optimizer.hpp:223-251); ccost/partial [N], hyper [N][W]; any may
 * be NULL.  The device does not store a HyperCache: hyper[p] = legs(p) & legs(c0) & legs(c1)
 * (infinite_memory/utils.hpp:82-91) is a function of the legs, derived by the kernels where
 * they need it and here on the host. */
int tnco_hip_get_caches(tnco_hip_handle h, int64_t replica, double* ccost, double* partial,
                        uint64_t* hyper);

/* is_valid(atol) for every replica, recomputed from scratch on the device
 * (optimizer.hpp:223-251).  n_bad = number of replicas failing; first_bad = one
 * of them or -1. */
int tnco_hip_validate(tnco_hip_handle h, double atol, int64_t* n_bad, int64_t* first_bad);

/* Diagnostics (no reference counterpart; the tests of tnco_hip_validate damage a replica with it and restore it): one
 * field of one replica is read and, when write != 0, replaced -- from the host (the handle is synchronised, the bytes
 * are copied; no kernel), at the address the getters above decode.  *previous (may be NULL) receives the value the
 * field held.  Costs travel as the bits of a double, mask words as they are, node ids and jmin as integers; a cached
 * width as the bits of a double whatever the width type (a float32 width is converted both ways).
 *   field                          node            word      value
 *   PARENT                         any node        -         an INTERNAL node id (n_leaves <= value < N; -1 at the root)
 *   SWAP_CHILDREN                  internal        -         -  (the left and right link words change places; previous = 0)
 *   LEGS                           internal        < W       mask word
 *   CCOST, PARTIAL                 internal        -         cost      (unified and split layouts)
 *   PARTIAL_LEFT, PARTIAL_RIGHT    internal        -         cost      (child-partial layout)
 *   TOTAL                          -               -         cost      (child-partial layout: the root's partial cost)
 *   MIN_COST                       -               -         cost      (min_total_cost)
 *   JMIN                           -               -         length of the journal prefix that makes the best tree
 *   SLICES, MIN_SLICES             -               < W       mask word (finite width)
 *   WIDTH                          internal        -         width     (finite width: the cached width of the node)
 * EINVAL, and nothing written, for: an index out of range; a field the handle's layout does not store (CCOST / PARTIAL
 * under child partials, PARTIAL_LEFT / PARTIAL_RIGHT / TOTAL elsewhere, SLICES / MIN_SLICES / WIDTH without max_width);
 * and every value that would let tnco_hip_validate's kernels walk off a tree -- they trust the child links while they
 * traverse.  So child links change only by SWAP_CHILDREN (still a binary tree), a parent is an existing internal node,
 * and JMIN stays within the rotations the journal holds (any prefix of them is a sequence of legal rotations from the
 * checkpoint: a test lowers it and puts the old value back). */
#define TNCO_HIP_POKE_PARENT 0
#define TNCO_HIP_POKE_SWAP_CHILDREN 1
#define TNCO_HIP_POKE_LEGS 2
#define TNCO_HIP_POKE_CCOST 3
#define TNCO_HIP_POKE_PARTIAL 4
#define TNCO_HIP_POKE_PARTIAL_LEFT 5
#define TNCO_HIP_POKE_PARTIAL_RIGHT 6
#define TNCO_HIP_POKE_TOTAL 7
#define TNCO_HIP_POKE_MIN_COST 8
#define TNCO_HIP_POKE_JMIN 9
#define TNCO_HIP_POKE_SLICES 10
#define TNCO_HIP_POKE_MIN_SLICES 11
#define TNCO_HIP_POKE_WIDTH 12
int tnco_hip_diag_poke(tnco_hip_handle h, int64_t replica, int field, int64_t node, int64_t word, int write,
                       uint64_t value, uint64_t* previous);

/* prng_state property / string-seed constructor (optimize/optimizer.hpp:68-71,
 * 191-195): 624 state words followed by the position, exactly the numbers
 * `oss << std::mt19937` prints. */
int tnco_hip_get_prng(tnco_hip_handle h, int64_t replica, uint32_t* state625);
int tnco_hip_set_prng(tnco_hip_handle h, int64_t replica, const uint32_t* state625);
/* The same for k replicas in one call: states [k][625]; replicas == NULL means replicas 0 .. k-1. */
int tnco_hip_get_prng_many(tnco_hip_handle h, int64_t k, const int64_t* replicas, uint32_t* states625);
int tnco_hip_set_prng_many(tnco_hip_handle h, int64_t k, const int64_t* replicas, const uint32_t* states625);

/* The k replicas of lowest min_total_cost, ascending, ties by replica id
 * (replaces `sorted(results)` of tnco/app/infinite_memory/sa.py:257 for the
 * head of the list).  k <= 2048: selected on the device (per-block bitonic sort + merge passes),
 * only the k pairs are copied back; longer heads sort the replica records on the host. */
int tnco_hip_best(tnco_hip_handle h, int64_t k, double* costs, int64_t* replicas);
/* min over the replicas of min_total_cost, reduced on the device into *device_dst_f64 (device
 * memory, e.g. a torch tensor's storage): the operand of the RCCL all-reduce(min) that replaces
 * the `sorted(results)[0]` of sa.py:257 across GPUs -- no host round trip. */
int tnco_hip_min_cost_device(tnco_hip_handle h, void* device_dst_f64);
/* ctree / min_ctree (optimize/optimizer.hpp:207-208) of k replicas in ONE buffer, and
 * get_contraction (include/tnco/utils.hpp:53-71) of each, computed on the device:
 * links [k][3][N] (left, right, parent); contraction [k][n_leaves-1][3] = (child0, child1, node)
 * per internal node in the post-order of utils.hpp:34-51, or NULL. */
int tnco_hip_get_trees(tnco_hip_handle h, int64_t k, const int64_t* replicas, int which, int32_t* links,
                       int32_t* contraction);
/* ContractionTree.path() (tnco/ctree.py:350-388) for k contractions of one component (host code):
 * tensors_pos[nc] = ascending positions of the component's tensors among all n_tensors
 * (`_tensors_pos`, ctree.py:128-132); contraction as tnco_hip_get_trees returns it; paths
 * [k][nc-1][2] linear (einsum) format, operand positions in the order (child0, child1). */
int tnco_hip_linear_paths(int32_t n_tensors, int32_t nc, const int32_t* tensors_pos, int64_t k,
                          const int32_t* contraction, int32_t* paths, int32_t n_threads);
/* merge_contraction_paths (tnco/utils/tn.py:334-401) for k results (host code): triples [k][steps][3]
 * = the components' contractions concatenated, in SSA form over all tensors (leaves 0..n_tensors-1,
 * step s creates id n_tensors + s); paths [k][steps][2], each pair sorted. */
int tnco_hip_linear_paths_ssa(int32_t n_tensors, int32_t steps, int64_t k, const int32_t* triples,
                              int32_t* paths, int32_t n_threads);

/* Work counters summed over replicas: move evaluations (iterations of the
 * while loop at optimizer.hpp:117-192), accepted moves, best-tree updates, and
 * moves whose (D, E) order was drawn at random (optimize/optimizer.hpp:135-141).
 * Any pointer may be NULL. */
int tnco_hip_diag_counters(tnco_hip_handle h, uint64_t* moves, uint64_t* accepted,
                          uint64_t* improved, uint64_t* random_picks);
/* Number of whole-tree copies taken for min_ctree (summed over replicas).  The
 * reference copies the tree on EVERY improvement (optimizer.hpp:198-201); this
 * build journals rotations and copies only after a journal overflow. */
int tnco_hip_diag_full_copies(tnco_hip_handle h, uint64_t* n);
/* Per replica move counter ([n_replicas]). */
int tnco_hip_diag_moves(tnco_hip_handle h, uint64_t* moves_per_replica);
/* Diagnostic (no reference counterpart): shader cycles per stage of the sweep
 * loop summed over replicas -- [mt19937, state branches, landing fence, store
 * phase, loop iterations].  All zero unless the library was built with
 * -DTNCO_PROFILE (`make -C tnco_amd/csrc profile`, tools/stage_cycles.py); with a finite-width
 * handle the slots are [too-wide counts, post-order, get_slices, rebuild + commit, re-slices]. */
int tnco_hip_diag_stage_cycles(tnco_hip_handle h, uint64_t* out5);

/* Device time of the kernels launched by tnco_hip_run / tnco_hip_run_fw since the last reset (HIP
 * events on the handle's streams), and the number of schedule chunks launched (one per call unless the
 * schedule is very long).  A handle that splits its steps over two streams (tnco_hip_diag_launch_groups() > 1)
 * reports the time from the first launch after the reset to the end of the last one: its concurrent
 * launches overlap, their durations do not add up. */
int tnco_hip_diag_kernel_time(tnco_hip_handle h, double* ms, int64_t* launches, int reset);
/* The same time split by kernel: [0] sa_run_kernel (Optimizer::update, infinite memory),
 * [1] the moves of the finite-width optimizer (finite_width/greedy/optimizer.hpp:130-331), [2] its re-slice
 * (:359-389: get_slices, the cost cache rebuilt or re-priced, the end of the sweep), [3] what orders the too-wide
 * tensors for get_slices (greedy/utils.hpp:62: fw_walk2_kernel; 0 when the whole re-slice of a
 * replica is one wavefront of fw_wave_kernel: counted under [2]); launches4 = launches of each -- for a finite-width
 * handle that runs its halves on two streams, launches PER STREAM (every event is one launch on each stream; the counts
 * are whole numbers because both streams launch the same sequence).  Either array ([4]) may be NULL. */
int tnco_hip_diag_kernel_times(tnco_hip_handle h, double* ms4, int64_t* launches4, int reset);

/* Concurrent launches a step of tnco_hip_run is split into (1, or 2 when there are more workgroups than resident ones: see
 * tnco_hip_run).  0: the handle keeps its trees in LDS during a launch (csrc/sa_small.h; the fast cost path only: uniform
 * power-of-two dims, float64, no sparse legs, no best trees handed in) -- without hyper-indices trees of up to 64 leaves and
 * 128 indices whatever the number of replicas, up to 128 leaves while the CUs hold the replicas in two rounds of 32 per CU, and
 * any tree of up to 1024 indices (at most 32 per tensor) when the whole batch fits the CUs' LDS at once (512 leaves: 512
 * replicas).  There are no workgroups of node blocks to split.  Same results either way, bit for bit. */
int tnco_hip_diag_launch_groups(tnco_hip_handle h);

/* Bytes of device memory held by the handle. */
int64_t tnco_hip_diag_device_bytes(tnco_hip_handle h);

/* Use an existing hipStream_t (e.g. torch's current stream) instead of the
 * handle's own. NULL restores the private stream. */
int tnco_hip_set_stream(tnco_hip_handle h, void* hip_stream);

void tnco_hip_destroy(tnco_hip_handle h);
/* The device memory of a destroyed handle (blocks of 1 MB and more) is kept for the next tnco_hip_create
 * of the process -- a job that builds optimizer after optimizer asks for the same sizes again, and
 * hipMalloc right after hipFree of ~10 GB sporadically took seconds (csrc/dev_cache.h; bounded by
 * TNCO_HIP_CACHE_MB, default min(an eighth of the device's memory, 32 GB), 0: off; emptied when ANY device
 * allocation of this library fails, which is then retried).  Other allocators of the process (PyTorch,
 * RCCL) cannot reach into it: CALL tnco_hip_release_cached BEFORE HANDING THE GPU TO ANOTHER ALLOCATOR.
 * tnco_hip_release_cached gives everything back now; tnco_hip_diag_cached_bytes: how much is held. */
void tnco_hip_release_cached(void);
uint64_t tnco_hip_diag_cached_bytes(void);

/* Host helper replacing the per-run call
 * get_random_contraction_path(...) + ContractionTree(path, ...)
 * (tnco/app/infinite_memory/sa.py:173-190, tnco/utils/tn.py:109-273,
 * tnco/ctree.py:108-251) for a batch: one seeded random initial tree per
 * replica for ONE connected component, written as links [R][3][N].
 * holders_off[n_inds+1] / holders[] = CSR list of the (ascending) leaves
 * holding each index.  Algorithm documented in tnco_amd/ctree.py
 * random_contraction (random Kruskal over a seeded index permutation). */
int tnco_hip_random_trees(int32_t n_leaves, int32_t n_inds, const int32_t* holders_off,
                          const int32_t* holders, int64_t n_replicas, const uint32_t* seeds,
                          int32_t* links_out, int32_t n_threads);

/* The same batch as the REFERENCE draws it (tnco/utils/tn.py:189-230): CPython's
 * Random(seed).shuffle of the component's tensors, then opt_einsum's greedy path finder with every
 * dimension 2 (restated: opt_einsum is not pinned by the reference and absent here -- "parity
 * unpinned"; spec in tnco_amd/ctree.py greedy_contraction).  output_mask ([W] or NULL): the output
 * indices held by at most one tensor (tn.py:175-178 drops the others).  draws ([n_replicas] or
 * NULL): in = 32-bit outputs of Random(seed) already consumed by earlier components of the same run
 * (the reference shares one generator over the components, tn.py:163), out = consumed after this
 * one. */
int tnco_hip_greedy_trees(int32_t n_leaves, int32_t n_inds, const int32_t* holders_off,
                          const int32_t* holders, const uint64_t* output_mask, int64_t n_replicas,
                          const uint32_t* seeds, uint64_t* draws, int32_t* links_out,
                          int32_t n_threads);

/* The same trees drawn ON THE DEVICE (csrc/greedy_device.hip: CPython's generator one lane per tree,
 * the greedy path finder one wavefront per tree -- over a multigraph held in LDS where the network has no
 * hyper-index, over index sets in memory otherwise); the trees come back in links_out (host memory).
 * Networks outside the kernel's limits (tnco_hip_diag_greedy_device_supported == 0: more than 2040
 * indices or 2000 tensors, an index held by more than 6 tensors) and single trees that end in outer
 * products are done by tnco_hip_greedy_trees on n_threads host threads: same result either way.
 * links_out (host, may be NULL) receives the trees; links_device (may be NULL) receives a pointer to
 * the same [n_replicas][3][N] array in DEVICE memory, which tnco_hip_create takes as tnco_hip_desc.links
 * without a copy or a host-side check (it validates the trees on the device).  That memory belongs
 * to the library: it stays valid until the next tnco_hip_greedy_trees_device call or
 * tnco_hip_greedy_device_release(). */
int tnco_hip_greedy_trees_device(int32_t device, int32_t n_leaves, int32_t n_inds, const int32_t* holders_off,
                                 const int32_t* holders, const uint64_t* output_mask, int64_t n_replicas,
                                 const uint32_t* seeds, uint64_t* draws, int32_t* links_out,
                                 int32_t** links_device, int32_t n_threads);
/* device -> host copy of such a buffer */
int tnco_hip_copy_to_host(void* dst, const void* device_src, uint64_t bytes);
/* host -> device copy into such a buffer (diagnostics: the tests plant damaged trees in it; the pointer must be one
 * this library handed out -- memory of another HIP runtime in the process, a torch tensor's, is not known to this one) */
int tnco_hip_copy_to_device(void* device_dst, const void* src, uint64_t bytes);
int tnco_hip_diag_greedy_device_supported(int32_t n_leaves, int32_t n_inds, const int32_t* holders_off);
/* diagnostics: the 36-bit key of the cost 2^a - 2^b - 2^c by which the device generator orders its
 * candidates (larger cost <=> larger key; a, b, c <= 2040) */
uint64_t tnco_hip_diag_greedy_cost_key(int32_t a, int32_t b, int32_t c);
/* the device memory tnco_hip_greedy_trees_device keeps between calls (one block, re-used) is freed */
void tnco_hip_greedy_device_release(void);
/* diagnostics: trees of the last device call that the host version did (-1: the whole batch) */
int64_t tnco_hip_diag_greedy_device_redone(void);
/* diagnostics: what the last tnco_hip_greedy_trees_device call launched (values the host computed for the launch, nothing
 * read back from a kernel but the statuses it reads anyway).  out8[0] form: 0 = the whole batch went to the host version,
 * 1 = set form (greedy_kernel), 2 = graph form (greedy_graph_kernel); [1] ROWS of the instantiation launched (set form:
 * 0 = the queue in LDS); [2] shuffle kernel: 0 = state in memory (py_shuffle_kernel), else the trees per workgroup of
 * py_shuffle_lds_kernel (8 or 16); [3] G, the wavefronts launched (each works through the trees g, g + G, ...);
 * [4] LDS bytes per wavefront of the greedy kernel; [5] R, the trees asked for; [6] trees the host version redid (-1:
 * the whole batch); [7] bit s set: some tree ended with status s (0 = done by the kernel; 3 = outer products left,
 * 7 = a neighbour list past its capacity, 9 = a merged tensor or a pair's shared legs past 255; 4, 5, 6: internal limits
 * of the set form).  Form 0: [1]..[4] and [7] are 0. */
int tnco_hip_diag_greedy_device_last(int64_t* out8);

/*
 * The exchange between the GPUs of one node -- replaces what little tnco/parallel.py:330-341 moves between its worker
 * processes (the results; here: the best cost, the heads of the result lists).  One process per GPU; RCCL over xGMI,
 * loaded with dlopen from the ROCm installation, i.e. on this library's own HIP runtime.  Rendezvous: rank 0 calls
 * tnco_hip_comm_unique_id and hands the 128 bytes to the other ranks by any means (tnco_amd/parallel.py: over TCP,
 * on the side channel the ranks share); then every rank calls tnco_hip_comm_init (collective).
 */
typedef struct tnco_hip_comm_s* tnco_hip_comm;
int tnco_hip_comm_unique_id(uint8_t* id128);
int tnco_hip_comm_init(int rank, int world, const uint8_t* id128, int device, tnco_hip_comm* out);
void tnco_hip_comm_destroy(tnco_hip_comm c);
/* min over the ranks of the best min_total_cost (replaces `sorted(results)[0]`, sa.py:257, across GPUs): the handle's
 * replicas are reduced on the device straight into the operand of ncclAllReduce(ncclMin) -- 8 bytes over xGMI, no host
 * round trip before the collective.  h == NULL: `local` is this rank's value instead. */
int tnco_hip_comm_allreduce_min(tnco_hip_comm c, tnco_hip_handle h, double local, double* out_min);
/* every rank's `bytes` bytes to every rank, in rank order: recv holds world * bytes */
int tnco_hip_comm_allgather(tnco_hip_comm c, const void* send, void* recv, uint64_t bytes);
int tnco_hip_comm_barrier(tnco_hip_comm c);
const char* tnco_hip_comm_last_error(void);

/*
 * Sliced pairwise contraction of arrays along a linear path (tnco/utils/tn.py:906 `contract(..., arrays=...)`, with
 * the slices of a finite-width result).  The plan is built by tnco_amd/contraction.py and handed over as flat int64
 * tables; tnco_hip_contract_run runs every slice assignment of [slice_start, slice_stop) and every step of the path in
 * one call, on one stream, and sums the assignments in that order (bit-reproducible).
 *
 * Kinds of an operand or destination: 0 a leaf (ref: leaf number), 1 the arena (ref: element offset), 2 the output
 * (the block of the current assignment).  Tables, row-major, max_axes = 32:
 *   leaf_sl [n_leaves][1 + 2 max_axes]  number of sliced axes, their slice positions, their element strides;
 *   perms   [n_perms][8 + 2 max_axes]   src kind, src ref, dst kind, dst ref, ndim, numel, group, 0, dims, src strides
 *                                      (group -1: gathered at the start of an assignment, one launch for all; k: before
 *                                      step k; rows sorted by group);
 *   steps   [n_steps][16]              A kind, ref, stride m, stride k; B kind, ref, stride k, stride n; C kind, ref;
 *                                      H, M, N, K; 0, 0.  Z[h][m][n] = sum_k A[h][m][k] B[h][k][n], operands dense per
 *                                      batch (A strides (K, 1) or (1, M), B (N, 1) or (1, K)), C dense [h][m][n].
 * The output buffer is [block slices][the rest]: block_slices lists the slice positions whose value selects a block.
 *
 * Row axes (projections of sparse indices): a tensor that holds sparse indices carries one outermost axis, a row per
 * distinct projection of those indices; the permute table sees it as an ordinary axis.  Two more tables say how the
 * rows of a step's operands meet:
 *   row_steps [n_steps][5]             R, rows of A, map of A, rows of B, map of B.  The result has R rows and
 *                                      Z[r][h][m][n] = sum_k A[a_map[r]][h][m][k] B[b_map[r]][h][k][n]; a map is an
 *                                      offset into row_maps (R entries, each below the operand's row count) or -1: the
 *                                      operand then has R rows, read in place, or one row, read for every r.
 *                                      Operands are dense [rows][h] batches, C dense [r][h][m][n].
 *   row_maps  [n_row_maps] int32       the pool of the maps.
 * row_steps == NULL (and n_row_maps == 0): no step has a row axis; a row of (1, 1, -1, 1, -1) says the same of one step.
 *
 * Storage mode, dtype codes 4..7: leaves and arena hold 16-bit values, every step sums in float32 and rounds once, to
 * nearest even, when it stores to the arena; the output is float32 / complex64 (beta and block placement in float32):
 *   4 float16 -> float32;  5 float16 pairs (re, im) -> complex64;  6 bfloat16 -> float32;  7 bfloat16 pairs -> complex64.
 * The leaves passed to tnco_hip_contract_run are in storage layout, `out` is float32 / complex64; arena_elems, leaf_numel
 * and every offset of the tables count storage elements (a pair is one element).  row_steps must be NULL (EINVAL).  No
 * scaling unless `scaling` is set: a sum beyond the storage type's range is stored as inf.  The launch slots keep their
 * meaning (shape class and operand layout of the step); the four tiled slots then count launches of the MFMA kernel.
 *
 * Per-tensor scaling, scaling = 1 (storage dtypes only, EINVAL otherwise): every stored tensor T, leaf or intermediate, has
 * one int32 exponent e in a device array of n_leaves + n_steps slots (leaf t: slot t; the result of step j: slot
 * n_leaves + j); its 16-bit values are round_nearest_even(x 2^-e) and mean stored 2^e.  e = floor(log2 m) - 14 with m the
 * largest |part| over the finite parts of the whole tensor, from the float32 bit pattern (subnormals included); e = 0 when
 * m == 0 or no part is finite.  The leaves come scaled from the host with their exponents (tnco_hip_contract_set_exponents).
 * Columns 14 and 15 of a steps row are the exponent slots of A and of B.  A step for the arena sums its stored operands in
 * float32 into a staging buffer of the arena (stage_refs[k]: its offset in storage elements, a multiple of 8; it takes
 * 2 H M N of them), the largest finite |part| is taken with an integer max over the bit patterns, and a narrowing pass
 * stores round(acc 2^-s) with e_C = e_A + e_B + s, s the rule applied to the sums.  The step for the output adds or places
 * ldexpf(acc, e_A + e_B); a single leaf gathered into the output is widened and scaled the same way.  Permutes move 16-bit
 * values as they are.  Exponents are recomputed in every slice assignment; nothing synchronises with the host in a run.
 *
 * Slice batches (tnco_hip_contract_set_slice_batch): with a batch of B the run takes the assignments in groups of up to
 * B consecutive numbers, the first group starting at slice_start, the last one possibly partial, and every step of the
 * path is one launch per group: member b of a group (assignment first + b) is one plane of the grid and works in its own
 * copy of the arena, at arena + b arena_elems, and with scaling in its own copy of the exponent slots and max words (the
 * leaves' exponents the same in every copy).  The tables are those of the unbatched plan.  The last step writes the
 * members' blocks, unrounded and with beta 0, to a staging buffer [B][block] of the output's type, and one more kernel per
 * group adds or places them in the output, one lane per element, the members in assignment order: the sum over the
 * assignments keeps its order, and the result is bit for bit that of the unbatched run.  Steps with row axes are not
 * supported.  A plan without steps takes the call and runs as it does without it.
 *
 * Compute mode bf16x3 (tnco_hip_contract_set_compute, mode 1; dtype codes 0 and 2 only): nothing changes in what is
 * stored, the tables or the memory; a step of the tiled shape class (M, N >= 64, K > 32) runs on the matrix cores with
 * every float32 part x of its operands split, as it is staged, into hi = bf16(x) (to nearest even) and lo = bf16(x - hi)
 * (exact subtraction; lo = 0 where hi is not finite), and every product summed in float32 as a_lo b_hi + a_hi b_lo +
 * a_hi b_hi, in that order, a_lo b_lo dropped (v_mfma_f32_16x16x32_bf16; a complex product: re += Ar Br, re += (-Ai) Bi,
 * im += Ar Bi, im += Ai Br, each as those three).  The result is stored unrounded as float32; no atomics, a run stays
 * bit-reproducible.  Every other kernel is that of mode 0.  A finite part with |x| >= 2^128 - 2^119 has an infinite hi:
 * the elements it feeds become non-finite (the host refuses such leaves).  Works with slice batches.
 *
 * Matrix mode (tnco_hip_contract_set_matrix; dtype codes 0..3): nothing changes in what is stored, the tables or the
 * memory; a step of the tiled shape class (M, N >= 64, K > 32) runs on the matrix cores in the element type's own
 * precision, a real product as v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64: an fma chain of that type, one rounding
 * per product, nothing rounded or split on the way.  An element is summed over k in blocks of 16, ascending, and in a
 * block in the order 0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15 (the plain tiled kernel: k ascending), so the
 * bits differ from mode off while the error bound is the same; a complex product at every such k: re += Ar Br,
 * re += (-Ai) Bi, im += Ar Bi, im += Ai Br.  The result is stored unrounded; no atomics, a run stays bit-reproducible.
 * Every other kernel is that of a handle without the call.  Exclusive with compute mode 1 and the path kernel; steps with
 * row axes and storage dtypes are not supported.  Works with slice batches and hoisting.
 *
 * Path kernel (tnco_hip_contract_set_path_kernel; dtype codes 0..3 only): with a group of G the run takes the assignments
 * in groups of up to G consecutive numbers, the first group starting at slice_start, the last one possibly partial, and a
 * group is two launches.  In the first, one workgroup per member (block b: assignment first + b) interprets the whole
 * path in its own copy of the arena, at arena + b arena_elems: permute group -1, then for each step its permute group
 * and the step, a workgroup barrier between consecutive operations; leaves are read in place at the slice offset of the
 * member's assignment.  A step sums in the order of the kernel the unfused loop launches for its shape (tiled and stream
 * class: k ascending per element; dot class: 256 partials per element and their tree).  The last step writes the
 * member's block, unrounded and with beta 0, to a staging buffer [G][block] of the output's type; the second launch adds
 * or places the blocks in the output, one lane per element, the members in assignment order, from a device table of
 * block offsets and beta bits that is filled for the whole run beforehand.  The result is bit for bit that of the unfused
 * run.  The tables are those of the plan; steps, the permute groups and the placement table are copied to the device in
 * addition.  A step may have 2^24 multiply-adds (H M N K) at most: one workgroup runs it.  Steps with row axes, storage
 * dtypes, slice batches and compute modes are not supported.  A plan without steps takes the call and runs as it does
 * without it.
 *
 * Hoisting (tnco_hip_contract_set_hoist): a step or a permute whose operands do not depend on the assignment -- no leaf
 * below them holds a sliced axis -- is flagged by the plan and runs once per run, before the first assignment, instead of
 * once per assignment: first the flagged rows of permute group -1, then for each step k the flagged rows of its permute
 * group and the step itself when it is flagged, as one-member launches of the kernels the loop would launch.  The loop
 * over the assignments skips what is flagged.  The flags are the two-period case of the schedule that Reuse (below)
 * describes, and one loop runs both: a flagged item has the period that is due at slice_start only (the number of
 * assignments), every other item has period 1, so the flagged items are the slow phase of the first assignment.
 * A flagged item reads leaves without sliced axes and arena tensors that
 * flagged items wrote, and writes the arena; what an unflagged step reads of it (a kept tensor) stays where it is for the
 * whole run, and the plan places nothing an assignment writes over it.  With a slice batch the flagged items work in arena
 * copy 0 and every member reads a kept tensor there; with scaling the exponent slots of copy 0 are copied to every member's
 * slots after the flagged items, in stream order.  Every step runs the kernel it runs unhoisted on the same operands, so
 * the result is bit for bit that of a handle without the call; stats[0] and the launch counts are of what ran.
 * The flags are refused in three places where the equal periods are not.  (a) A flagged item must not read a leaf with
 * any sliced axis; a period only counts the axes of a dimension above 1.  (b) A flagged step must not read an arena
 * tensor that no item wrote.  (c) A permute and the item that wrote its source carry the same flag; periods let a permute
 * be faster than its source, which is then kept.  (c) is what makes a slice batch sound, which flags accept and periods
 * do not: only a step operand can be marked as kept and read in arena copy 0 by every member, so an unflagged permute of a
 * kept tensor would read the arena copy of its own member, where nothing wrote it.
 *
 * Reuse (tnco_hip_contract_set_reuse): hoisting with as many levels as there are sliced indices.  Assignment a gives
 * sliced index j the value (a / place[j]) % dim[j], place[j] the product of the dimensions after j, so a tensor whose
 * leaves hold the sliced indices D has one value for all a with equal a / min place[D] (a / number of assignments when D
 * is empty).  The plan gives every step and permute that number as its period, and an item runs at assignment a iff a
 * is slice_start or a % period == 0.  The items of one period are a phase; at an assignment the phases that are due run
 * one after the other, the largest period first, each as the plain loop runs an assignment: the rows of permute group -1
 * of that period (one gather launch, sized by the largest of them), then for each step k the rows of its group of that
 * period and the step itself when it has that period.  A tensor whose reader has a smaller period than its writer is
 * kept: it stays where it is until its writer is due again.  A slower phase may use the room of a faster phase's kept
 * tensors for its temporaries -- whenever it is due, every faster phase is due after it and writes them again -- which
 * is why the phases do not interleave in path order.  With scaling the exponent slot of a kept tensor stays as written;
 * an assignment clears the max words only.  Every step runs the kernel it runs in the plain loop on the same operands,
 * so the result is bit for bit that of a handle without the call; stats[0] and the launch counts are of what ran.
 * Works with storage dtypes, scaling, compute mode 1, matrix mode and indirect operands; not with row axes, slice
 * batches, the path kernel or hoisting (which is its two-level case).
 *
 * Indirect operands (tnco_hip_contract_set_indirect; dtype codes 0..3 only): a step operand that the plan folded is not
 * permuted into the dense [h][m][k] / [h][k][n] order; it stays where it lies -- a leaf, also one that is not dense after
 * slicing, read at the slice offset of the assignment, or the arena tensor an earlier step left -- and the step reads its
 * element (h, m, k) at base + offH[h] + offM[m] + offK[k] (B: offH[h] + offK[k] + offN[n]), three int64 tables of element
 * offsets per operand in one pool.  Both stride columns of such an operand in `steps` are 0 (create accepts that; a run
 * of such a handle without the tables is EINVAL), and two tables say where its offsets are:
 *   ind_steps [n_steps][6]             offsets into ind_maps of the tables of A by h, m, k and of B by h, k, n (H, M, K /
 *                                      H, K, N entries); the three of an operand that is not folded are -1;
 *   ind_maps  [n_maps] int64           the pool.
 * A step with a folded operand runs a twin of the plain kernel of its shape class (contract_indirect.h), every element
 * the same products in the same order, so the result is bit for bit that of the plan that permutes.  Works with slice
 * batches and hoisting; steps with row axes, storage dtypes, compute mode 1, matrix mode and the path kernel are not
 * supported.
 *
 * Wide accumulation (tnco_hip_contract_set_accumulate; float32 / complex64 outputs: dtype codes 0, 2 and 4..7): the
 * blocks of the slice assignments, each computed as without the call, are summed in float64 / complex128 in assignment
 * order and rounded once into the output (contract_accumulate.h; the call's own comment below has the definition).  Works
 * with everything above except row axes.
 */
typedef struct tnco_hip_contract_s* tnco_hip_contract;
typedef struct tnco_hip_contract_desc {
  int32_t dtype;            /* 0 float32, 1 float64, 2 complex64, 3 complex128 (interleaved); 4..7: storage mode, above */
  int32_t device;
  int64_t max_axes;         /* must be 32 */
  int64_t n_leaves;
  const int64_t* leaf_numel;
  const int64_t* leaf_sl;
  int64_t n_perms;
  const int64_t* perms;
  int64_t n_steps;
  const int64_t* steps;
  int64_t arena_elems;
  int64_t out_numel;        /* the whole output, every block */
  int64_t n_slice_dims;
  const int64_t* slice_dims;  /* the first one the most significant digit of an assignment number */
  int64_t n_block;
  const int64_t* block_slices;
  int64_t slice_start;
  int64_t slice_stop;
  const int64_t* row_steps;  /* NULL: no row axes */
  int64_t n_row_maps;
  const int32_t* row_maps;
  int64_t scaling;           /* 0, or 1: per-tensor power-of-two scaling (storage dtypes only) */
  const int64_t* stage_refs; /* [n_steps] with scaling: arena offset of the step's float32 staging buffer, -1 for the output step */
} tnco_hip_contract_desc;
/* validates the plan, allocates leaves + arena + output on the device (ERUNTIME when they exceed its free memory) */
int tnco_hip_contract_create(const tnco_hip_contract_desc* d, tnco_hip_contract* out);
/* leaves: host pointers in the leaves' order (C-contiguous, dtype of the plan); out: host, out_numel elements */
int tnco_hip_contract_run(tnco_hip_contract h, const void* const* leaves, void* out);
/* stats[4]: multiply-adds launched by the last run, its kernel launches, device bytes reserved, device time of the
 * last run's kernels in ns (events around the slice loop: leaf copies in and the result copy out excluded) */
int tnco_hip_contract_stats(tnco_hip_contract h, int64_t* stats);
/* counts[TNCO_HIP_CONTRACT_N_KERNELS]: the last run's launches per kernel path; with the row-mapped paths below their sum
 * is stats[1].  Order:
 *   0 gather (slices + permutes);
 *   1..4 tiled GEMM by operand layout: 1 A [k][m], B [n][k];  2 A [k][m], B [k][n];  3 A [m][k], B [n][k];
 *        4 A [m][k], B [k][n]  (slot 1 + 2 (A contiguous along k) + (B contiguous along n));
 *   5 dot (K split over a block);  6 stream (one lane per output element). */
#define TNCO_HIP_CONTRACT_N_KERNELS 7
int tnco_hip_contract_kernel_launches(tnco_hip_contract h, int64_t* counts);
/* counts[TNCO_HIP_CONTRACT_N_ROW_KERNELS]: the last run's launches of the row-mapped GEMM paths (steps with a row axis);
 * stats[1] is the sum of these and of the seven above.  Order: 0 rows_tiled (any operand layout), 1 rows_dot,
 * 2 rows_stream. */
#define TNCO_HIP_CONTRACT_N_ROW_KERNELS 3
int tnco_hip_contract_row_launches(tnco_hip_contract h, int64_t* counts);
/* scaling: the leaves' exponents, n_leaves of them, for the runs that follow (zeros until set) */
int tnco_hip_contract_set_exponents(tnco_hip_contract h, const int32_t* exps);
/* scaling: the n_leaves + n_steps exponent slots as the last assignment of the last run left them (the slot of the
 * step that writes the output is not used and stays 0) */
int tnco_hip_contract_exponents(tnco_hip_contract h, int32_t* exps);
/* scaling: the last run's launches of the narrowing pass; they are part of stats[1] and of none of the slots above */
int tnco_hip_contract_narrow_launches(tnco_hip_contract h, int64_t* count);
/* after create, before run: the runs that follow take `batch` assignments per launch (above).  EINVAL for a batch
 * outside [1, 64] and on a handle with row axes.  Reserves `batch` arenas, the batch staging buffer of the output, and with
 * scaling `batch` copies of the exponent slots and max words (ERUNTIME when they exceed the device's free memory; the
 * handle then stays as it was); stats[2] counts them.  A handle on which this was never called runs unbatched.
 * tnco_hip_contract_exponents then gives the slots of the last member of the last group */
int tnco_hip_contract_set_slice_batch(tnco_hip_contract h, int64_t batch);
/* the last run's launches of the kernel that folds a group's blocks into the output (one per group; 0 unbatched); they
 * are part of stats[1] and of none of the slots above */
int tnco_hip_contract_batch_launches(tnco_hip_contract h, int64_t* count);
/* after create: the runs that follow use compute mode `mode`, 0 plain (as a handle on which this was never called) or
 * 1 bf16x3 (above).  EINVAL for other values, for dtype codes other than 0 and 2, and on a handle with row axes */
int tnco_hip_contract_set_compute(tnco_hip_contract h, int32_t mode);
/* the last run's launches of the split kernel of mode 1; they are also counted in their tiled slot of
 * tnco_hip_contract_kernel_launches (by operand layout), so the slots still sum to stats[1] as before */
int tnco_hip_contract_split_launches(tnco_hip_contract h, int64_t* count);
/* after create: on = 1: the runs that follow use matrix mode (above); on = 0: they do not, as on a handle on which this
 * was never called.  EINVAL for other values, on a handle with row axes, a storage dtype, compute mode 1 or a path
 * kernel; a handle with matrix mode on refuses compute mode 1 and a path kernel in turn */
int tnco_hip_contract_set_matrix(tnco_hip_contract h, int32_t on);
/* the last run's launches of the matrix kernel; they are also counted in their tiled slot of
 * tnco_hip_contract_kernel_launches (by operand layout), so the slots still sum to stats[1] as before */
int tnco_hip_contract_matrix_launches(tnco_hip_contract h, int64_t* count);
/* after create, before run, once per handle: the runs that follow take `group` assignments per launch of the path
 * kernel (above).  EINVAL for a group outside [1, 1024], on a handle with row axes, a storage dtype, a slice batch or a
 * compute mode, and when a step has more than 2^24 multiply-adds (the message names the step); a handle that took this
 * call refuses a slice batch and a compute mode in turn.  Reserves `group` arenas and the staging buffer of the output,
 * and uploads the steps, the permute groups and the placement of every assignment of [slice_start, slice_stop) (ERUNTIME
 * when they exceed the device's free memory; the handle then stays as it was); stats[2] counts them.  A handle on which
 * this was never called runs the unfused loop */
int tnco_hip_contract_set_path_kernel(tnco_hip_contract h, int64_t group);
/* counts[2]: the last run's launches of the path kernel and of the kernel that folds a group's blocks into the output
 * (one each per group; 0, 0 without a path kernel and for a plan without steps).  stats[1] is their sum, and every slot
 * of tnco_hip_contract_kernel_launches and tnco_hip_contract_row_launches is 0 on such a run */
int tnco_hip_contract_path_launches(tnco_hip_contract h, int64_t* counts);
/* after create, before run: step_flags[n_steps] and perm_flags[n_perms] (in the rows' order), 1 for what the runs that
 * follow do once per run instead of once per assignment (above), 0 for the rest.  EINVAL for a value other than 0 and 1,
 * on a handle with row axes or a path kernel (which refuses this handle in turn), for a flagged step that writes the
 * output or has an operand with a sliced axis or an arena operand that an unflagged item wrote, for a flagged permute
 * that writes the output or whose source has a sliced axis or was written by an unflagged item, for an unflagged permute
 * whose source a flagged item wrote, for a permute group whose flagged rows do not come first, and when an unflagged item
 * writes over a kept tensor.  The flags are checked as the periods of tnco_hip_contract_set_reuse are, a flag as the
 * number of assignments and no flag as 1, with the three further refusals listed under Hoisting above (a sliced axis of
 * dimension 1, an arena operand that nothing wrote, a permute that is faster than its source), which keep a flagged
 * handle fit for a slice batch.  Reserves nothing.  A handle on which this was never called, or with no flag set, runs
 * everything per assignment */
int tnco_hip_contract_set_hoist(tnco_hip_contract h, const int64_t* step_flags, const int64_t* perm_flags);
/* after create, before run: step_period[n_steps] and perm_period[n_perms] (in the rows' order), the period of every item
 * (above).  EINVAL, each with a text of its own and the handle left as it was: for a period that is neither the place of
 * a sliced index nor the number of assignments; on a handle with row axes, a path kernel, a slice batch or hoist flags
 * (each of those calls refuses a handle with periods in turn); for a step or permute that writes the output with a
 * period other than 1; for a permute group whose rows are not ordered by period, the largest first; for an item with a
 * larger period than a leaf it reads allows (the smallest place of the leaf's sliced axes of a dimension above 1) or
 * than the item that wrote its arena operand or source; and when an item writes into a kept tensor after its writer
 * in the writer's phase, or in any faster phase.  Reserves nothing.  A handle on which this was never called, or with every period 1, runs everything
 * per assignment */
int tnco_hip_contract_set_reuse(tnco_hip_contract h, const int64_t* step_period, const int64_t* perm_period);
/* after create, before run: the offset tables of the folded operands (above).  Validated on the host, so that no table
 * can send a lane outside its operand: EINVAL when a table does not lie inside the pool, an entry is negative, the base
 * plus the largest entries of an operand's three tables is not inside its leaf (at the largest slice offset) or the
 * arena, an operand has some of its three tables but not all, a folded operand has a stride column that is not 0 or an
 * operand without tables has both 0, or the result of the step overlaps what a folded arena operand reaches.  EINVAL,
 * each with a text of its own, on a handle with row axes, a storage dtype, compute mode 1, matrix mode or a path kernel;
 * a handle with tables refuses those three calls in turn.  Uploads both tables (ERUNTIME when they exceed the device's
 * free memory; the handle then stays as it was); stats[2] counts them.  With no operand folded the handle runs as one on
 * which this was never called */
int tnco_hip_contract_set_indirect(tnco_hip_contract h, const int64_t* ind_steps, int64_t n_maps, const int64_t* maps);
/* counts[TNCO_HIP_CONTRACT_N_IX_KERNELS]: the last run's launches of the kernels that read a folded operand: 0 ix_tiled,
 * 1 ix_dot, 2 ix_stream.  They are part of stats[1] and, like the row-mapped paths, of no slot of
 * tnco_hip_contract_kernel_launches */
#define TNCO_HIP_CONTRACT_N_IX_KERNELS 3
int tnco_hip_contract_indirect_launches(tnco_hip_contract h, int64_t* counts);
/* after create, before run: the runs that follow sum the blocks of the slice assignments in float64 (mode 1) or as a
 * handle on which this was never called (mode 0).  Mode 1: every assignment computes its block of the output as before,
 * the same kernels on the same shapes in the same k order, always with beta 0 and into a staging block (the batch
 * staging buffer, the path kernel's, or unbatched a block reserved here).  The blocks go in assignment order, each part
 * (re, im) on its own, into an accumulator of float64 / complex128 with one element per output element: the first block
 * that reaches an output block is placed, widened exactly, every later one added with one float64 addition.  After the
 * last assignment the accumulator is rounded once, to nearest even, into the output; blocks the run does not reach stay
 * zero.  No atomics, the order fixed: the result does not depend on a slice batch, the path kernel, hoist flags, periods
 * or indirect operands, and where every output block is visited once it is that of mode 0.  A plan without steps sums
 * nothing: it runs as in mode 0 and nothing is reserved.
 * EINVAL, each with a text of its own and the handle left as it was: a mode other than 0 and 1; dtype codes 1 and 3 (the
 * output must be float32 / complex64: codes 0, 2 and the storage dtypes); a handle with row axes.  Reserves the
 * accumulator and, without a slice batch and a path kernel, the staging block (ERUNTIME when they exceed the device's
 * free memory; the handle then stays as it was); stats[2] counts them.  May come before or after the other set calls: a
 * slice batch or a path kernel set later releases the staging block */
int tnco_hip_contract_set_accumulate(tnco_hip_contract h, int32_t mode);
/* counts[2]: the last run's launches of the kernels that fold blocks into the accumulator (one per assignment, per group
 * of a slice batch or of the path kernel) and of the kernel that rounds it into the output (one per run); zeros in mode
 * 0.  They are part of stats[1]; the folds are also counted by tnco_hip_contract_batch_launches (with a path kernel: in
 * slot 1 of tnco_hip_contract_path_launches), the rounding by tnco_hip_contract_narrow_launches */
int tnco_hip_contract_accumulate_launches(tnco_hip_contract h, int64_t* counts);
/* Resident use: one handle, many runs, leaves and result in host or in device memory.  tnco_hip_contract_run is "load
 * every leaf from the host, then run what is loaded"; the two halves are entry points of their own.
 *
 * A caller's device pointer is touched by kernels only.  A process that uses PyTorch holds two HIP runtimes, PyTorch's
 * bundled one and the one this library links, and memory that one of them allocated is unknown to the other: a copy, a
 * memset or an attribute query on it fails or worse.  So no API call of this library's runtime ever gets such a pointer:
 * it is an argument of ct_ingest_kernel / ct_emit_kernel (csrc/contract_io.h) and nothing else.  Two things follow.  The
 * library cannot tell what a device pointer can reach: the caller checks that dims and strides stay inside its
 * allocation.  And the two sides are ordered by full synchronisation, not by events: the caller's work on the memory has
 * finished before the call (for PyTorch: torch.cuda.synchronize), and each of these entry points synchronises the
 * handle's stream before it returns.
 *
 * load_leaf: leaf `leaf` of the plan from `src`, ndim <= 32 axes of `dims`.  where 0: host memory, C-contiguous
 * (strides == NULL), src_dtype the handle's dtype code (a storage code: storage layout), copied as tnco_hip_contract_run
 * copies it.  where 1: device memory, `strides` in elements, >= 0, 0 allowed (an expanded axis), NULL: C-contiguous;
 * src_dtype 0..3 the handle's dtype or one that widens to it exactly (float32 -> float64, complex64, complex128;
 * float64 -> complex128; complex64 -> complex128; a real source gives an imaginary part of +0.0).  A loaded leaf stays
 * until it is loaded again or the handle is destroyed.  EINVAL, each with a text of its own and the handle left as it
 * was: a null pointer; a leaf number outside the plan; `where` not 0 or 1; ndim outside [0, 32]; a dimension below 1; a
 * negative stride; dims whose product is not the leaf's leaf_numel; a host leaf of another dtype or with strides; a
 * device leaf on a handle with a storage dtype (4..7) or scaling; a src_dtype that does not widen to the handle's. */
int tnco_hip_contract_load_leaf(tnco_hip_contract h, int64_t leaf, const void* src, int32_t where, int32_t src_dtype,
                                int64_t ndim, const int64_t* dims, const int64_t* strides);
/* runs as tnco_hip_contract_run does once the leaves are in place.  where 0: `out` is host memory and gets the raw output
 * buffer, out_numel elements, [block axes][the other axes]; ndim, dims and dst_strides are not read.  where 1: `out` is
 * device memory; dims are those of the output buffer's axes in its own order, dst_strides (in elements) where each of
 * them goes in `out`.  EINVAL: a null pointer; `where` not 0 or 1; folded operands without their tables (as run); with
 * where 1 a handle with row axes, ndim outside [0, 32], a dimension below 1, a negative stride or one of 0 on an axis
 * longer than 1, dims whose product is not out_numel; a leaf that was never loaded (the text names the first one). */
int tnco_hip_contract_run_loaded(tnco_hip_contract h, void* out, int32_t where, int64_t ndim, const int64_t* dims,
                                 const int64_t* dst_strides);
/* counts[2]: launches of ct_ingest_kernel and of ct_emit_kernel since the handle was created; they are no part of
 * stats[1] or of any other counter, and the kernels reserve nothing: stats[2] does not change */
int tnco_hip_contract_io_launches(tnco_hip_contract h, int64_t* counts);
/* Leaf sets: many runs of one plan that differ in a few leaves, in one call (csrc/contract_sets.h).  On a handle with a
 * path kernel a member of a launch is a pair (leaf set i, assignment a), numbered set-major: with A = slice_stop -
 * slice_start, member m = i A + (a - slice_start).  A leaf that differs between the sets is loaded as a stack
 * [n_sets][leaf_numel] into a buffer of the handle's own, apart from the leaf's single buffer, which stays as it is; every
 * other leaf is read from its single buffer by every set.  The members run in groups of `group` consecutive ones, two
 * launches per group, and the output of set i is bit for bit that of tnco_hip_contract_run_loaded over leaf set i: the
 * blocks of a set are folded in ascending assignment order with the placement and beta bits of the path kernel's table.
 *
 * load_leaf_sets: tnco_hip_contract_load_leaf for a stack: the product of `dims` is n_sets leaf_numel, the elements in C
 * order of the dims are set 0, set 1, ...; where, src_dtype and strides as there (a stride of 0 on a set axis gives equal
 * sets).  A caller's device pointer is touched by ct_ingest_kernel only.  The stack stays until the next
 * tnco_hip_contract_run_sets has read it, or until the leaf's stack is loaded again; its buffer grows to the largest
 * n_sets loaded and stays until destroy (ERUNTIME when it exceeds the device's free memory; the handle then stays as it
 * was); stats[2] counts it.  EINVAL, each with a text of its own and the handle left as it was: a null pointer; a leaf
 * number outside the plan; n_sets < 1 or too large for 64-bit offsets; a handle with row axes, without a path kernel,
 * with wide accumulation or without steps; and what load_leaf refuses of where, ndim, dims, strides and src_dtype. */
int tnco_hip_contract_load_leaf_sets(tnco_hip_contract h, int64_t leaf, int64_t n_sets, const void* src, int32_t where,
                                     int32_t src_dtype, int64_t ndim, const int64_t* dims, const int64_t* strides);
/* runs the n_sets sets: a leaf whose stack holds n_sets sets is read from it at set stride leaf_numel, every other leaf
 * must be loaded and is read from its single buffer at set stride 0; min(group, n_sets A) members per launch.  where 0:
 * `out` is host memory and gets n_sets raw output buffers back to back, [n_sets][out_numel]; ndim, dims and dst_strides
 * are not read.  where 1: `out` is device memory, written by ct_emit_kernel with the set axis as one more axis: dims are
 * those of [n_sets][the output buffer's axes] in that order (axes may be merged; the product is n_sets out_numel),
 * dst_strides (in elements) where each of them goes in `out`.  Reserves, and keeps until destroy, the arenas and staging
 * blocks beyond the path kernel's group that the members need, n_sets output buffers, and a table of a pointer and a
 * stride per leaf (ERUNTIME when they exceed the device's free memory; the handle then stays as it was); stats[2]
 * counts them.  stats[0] is n_sets times a run's multiply-adds, stats[1] the launches, two per group.  A run reads the
 * stacks once: the next one needs them loaded again.  Synchronises the handle's stream before it returns.  EINVAL, each
 * with a text of its own and the handle left as it was: a null pointer; n_sets < 1 or too large; a group outside
 * [1, 1024]; a handle with row axes, without a path kernel, with wide accumulation or without steps; `where` not 0 or 1;
 * with where 1 what run_loaded refuses of ndim, dims and dst_strides; a leaf whose stack holds another number of sets
 * (the text names the leaf and both numbers); a leaf without a stack that was never loaded. */
int tnco_hip_contract_run_sets(tnco_hip_contract h, int64_t n_sets, int64_t group, void* out, int32_t where, int64_t ndim,
                               const int64_t* dims, const int64_t* dst_strides);
/* counts[2]: the last run's launches of ct_sets_path_kernel and of ct_sets_reduce_kernel (one each per group; 0, 0 after
 * any other run).  stats[1] is their sum, and every other launch counter is 0 after tnco_hip_contract_run_sets */
int tnco_hip_contract_sets_launches(tnco_hip_contract h, int64_t* counts);
/* Walkers: the state of a gate-by-gate circuit sampler on the device (csrc/contract_walk.h).  A walkers object is the
 * library's own and belongs to no contraction handle: `bits`, a uint8 table [n_qubits][n_walkers] (qubit-major), all 0
 * at creation; a `dead` flag per walker, 0 at creation; a 64-bit seed.  Every entry point synchronises before it
 * returns. Each refusal below has a text of its own, comes before any allocation and leaves the object as it was.
 *
 * create: EINVAL for a null pointer, n_walkers < 1, n_qubits < 1, more than 2^40 bits, a device that is not there;
 * ERUNTIME when the table exceeds the device's free memory.  destroy: NULL is fine. read: the table
 * [n_qubits][n_walkers] into bits_out and the flags [n_walkers] into dead_out, host memory; one of the two may be
 * NULL.  write: the table from bits_in, host memory; the flags stay; EINVAL for a byte that is not 0 or 1. reset:
 * every bit and every flag 0. */
typedef struct tnco_hip_walkers_s* tnco_hip_walkers;
int tnco_hip_walkers_create(int32_t device, int64_t n_walkers, int64_t n_qubits, uint64_t seed, tnco_hip_walkers* out);
void tnco_hip_walkers_destroy(tnco_hip_walkers w);
int tnco_hip_walkers_read(tnco_hip_walkers w, uint8_t* bits_out, uint8_t* dead_out);
int tnco_hip_walkers_write(tnco_hip_walkers w, const uint8_t* bits_in);
int tnco_hip_walkers_reset(tnco_hip_walkers w);
/* A classical gate on k <= 8 qubits (ct_walk_permute_kernel, one lane per walker): with v the number that a walker's
 * bits of qubits[0..k) spell, the first qubit the most significant, those bits become table[v].  EINVAL: a null
 * pointer; k outside [1, 8]; a qubit outside [0, n_qubits) or named twice; a table that is no permutation of 0 .. 2^k
 * - 1. */
int tnco_hip_walkers_permute(tnco_hip_walkers w, int64_t k, const int64_t* qubits, const uint8_t* table);
/* Indexed leaves.  load_leaf_versions: tnco_hip_contract_load_leaf_sets for the versions of a leaf,
 * [n_versions][leaf_numel] under its rules of where, src_dtype, ndim, dims and strides, into a buffer of the handle's
 * own apart from the leaf's single buffer and from its stack; n_versions must be 2.  The versions stay until they are
 * loaded again or the handle is destroyed: a run does not use them up.  stats[2] counts the buffer.  EINVAL as
 * load_leaf_sets, and n_versions != 2.
 *
 * run_walkers: tnco_hip_contract_run_sets with n_sets = n_walkers and no stacks: walker i reads leaf t with
 * leaf_qubit[t] = q >= 0 at the version bits[q][i] of its two versions, which must be loaded, and every other leaf
 * (leaf_qubit[t] = -1) from its single buffer, which must be loaded (ct_walk_path_kernel, then ct_sets_reduce_kernel;
 * min(group, n_walkers A) members per launch).  Output i is bit for bit that of tnco_hip_contract_run_loaded over the
 * leaves walker i selects.  The n_walkers outputs stay in the handle's set-output buffer, [n_walkers][out_numel],
 * until the handle's next run of any kind; nothing is copied to the caller.  Where no leaf is indexed no output
 * depends on the walker: one set is run (n_sets = 1 in every count), and its one output serves every walker.  Reserves
 * what run_sets reserves, and a table of three words per leaf (ERUNTIME when they exceed the device's free memory; the
 * handle then stays as it was).  stats and tnco_hip_contract_sets_launches count as after run_sets.  EINVAL, the
 * handle and the walkers left as they were: a null pointer; a group outside [1, 1024]; what run_sets refuses of the
 * handle; walkers on another device than the handle's; too many walkers for 64-bit offsets; a leaf_qubit outside [-1,
 * n_qubits) (the text names leaf and qubit); an indexed leaf without versions; another leaf that was never loaded.
 *
 * walkers_output: the outputs of the last run, [n_walkers][out_numel] raw output buffers ([1][out_numel] where no leaf
 * was indexed), into host memory: what a test or a caller that does not choose on the device reads.  EINVAL unless the
 * handle's last run was a run_walkers over `w`. */
int tnco_hip_contract_load_leaf_versions(tnco_hip_contract h, int64_t leaf, int64_t n_versions, const void* src,
                                         int32_t where, int32_t src_dtype, int64_t ndim, const int64_t* dims,
                                         const int64_t* strides);
int tnco_hip_contract_run_walkers(tnco_hip_contract h, tnco_hip_walkers w, const int64_t* leaf_qubit, int64_t group);
int tnco_hip_contract_walkers_output(tnco_hip_contract h, tnco_hip_walkers w, void* out);
/* The new bit of one qubit for every walker (ct_walk_choose_kernel, one lane per walker).  The handle's last run must
 * be a run_walkers over `w` whose output holds exactly 2 elements, the amplitudes a0, a1 of the qubit's two values.
 * In float64, every operation rounded on its own and none fused: p = re re + im im with the parts widened exactly (a a
 * for a real dtype), s = p0 + p1.  u comes from Philox4x32-10 with key (seed lo, seed hi) and counter (i lo, i hi,
 * step, 0) for walker i: u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 of its first two output words.  bits[qubit][i] = (u s
 * < p1).  Where s is 0 or not finite the bit becomes 0 and dead[i] is set.  No state is kept between draws: the choice
 * is a function of (seed, i, step, a0, a1).  EINVAL: a null pointer; a last run that was not a run_walkers over `w`;
 * an output of another size than 2; a qubit outside [0, n_qubits); a step outside [0, 2^32). */
int tnco_hip_walkers_choose(tnco_hip_walkers w, tnco_hip_contract h, int64_t qubit, int64_t step);
/* The new bits of k <= 6 qubits for every walker, drawn jointly (ct_walk_choose_joint_kernel, one lane per walker). The
 * handle's last run must be a run_walkers over `w` whose output holds exactly N = 2^k elements.  Outcome v, 0 <= v < N,
 * has qubits[0] as its most significant bit: bit_j(v) = (v >> (k - 1 - j)) & 1, and its amplitude a_v is the element
 * sum_j bit_j(v) strides[j] of the walker's output.  In float64, every operation rounded on its own: p_v as choose has
 * p; tail(N - 1) = p_{N-1}, tail(v) = tail(v + 1) + p_v, s = tail(0); u is choose's u for (seed, i, step), one draw
 * whatever k is; t = u s.  The outcome is the largest v >= 1 with t < tail(v), or 0 if there is none;
 * bits[qubits[j]][i] = bit_j of it.  Where s is 0 or not finite the k bits become 0 and dead[i] is set.  So an outcome
 * v >= 1 with p_v = 0 is never drawn, and outcome 0 with p_0 = 0 only where u s rounds up to s.  At k = 1 the bytes are
 * those of tnco_hip_walkers_choose.  EINVAL, checked in this order and before any launch: a null pointer; a last run
 * that was not a run_walkers over `w`; k outside [1, 6]; an output of another size than 2^k; a qubit outside [0,
 * n_qubits) or named twice; strides that are no permutation of 1, 2, ..., 2^(k-1); a step outside [0, 2^32). */
int tnco_hip_walkers_choose_joint(tnco_hip_walkers w, tnco_hip_contract h, int64_t k, const int64_t* qubits,
                                  const int64_t* strides, int64_t step);
void tnco_hip_contract_destroy(tnco_hip_contract h);

/* "name|pci ...|uuid ...|N CUs" of a device: what a multi-GPU bench line lists per rank */
int tnco_hip_device_name(int device, char* buf, int cap);
int tnco_hip_device_count(void);
const char* tnco_hip_last_error(void);
const char* tnco_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TNCO_HIP_H_ */
