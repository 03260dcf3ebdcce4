/*
 * moc_hip.h -- C ABI of libmoc_hip.so: the MI355X (gfx950) kernels for the hot
 * path of xmed-lab/MOC.
 *
 * The reference has no FFI of its own: its seam is a set
 * of Python callables in main_moc.py and utils/patch_selection_classifier*.py.
 * Each entry point below names the reference lines it replaces; the Python
 * package moc_amd binds them with ctypes (INTEGRATION.md shows the stub a
 * maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer marked "device" is HIP device memory owned by the caller
 *     (PyTorch tensors in practice); the compute entry points never allocate, free or
 *     keep device memory and hold no state between calls.  The ONE exception is the
 *     node-local exchange handle `moc_p2p_t` (moc_p2p_create ... moc_p2p_destroy, below):
 *     it owns its fine-grained receive buffers (hipExtMallocWithFlags), one pinned host
 *     error word, the peers' IPC mappings and a sequence counter -- allocation and state
 *     are confined to that handle, created and destroyed explicitly by the caller, and
 *     exist only in a multi-rank run ("no cross-call state except an
 *     optional handle for persistent-kernel resources");
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     every call returns without synchronising the host;
 *   - return value 0 = success; otherwise a MOC_E* code, with a message
 *     available from moc_last_error() (thread local);
 *   - all matrices are row-major and dense; bag rows must be 16-byte aligned
 *     (D*elem_size % 16 == 0 and a 16-byte aligned base);
 *   - "slot space": work arrays are indexed by slot, not by row of X; total_rows is the
 *     number of slots (sum of the batch's slide sizes).  The kept (un-masked) rows of slide b occupy slots
 *     [row_off[b], row_off[b] + n_kept[b]) of every per-row work array, in
 *     ascending row order; with no mask n_kept[b] == rows of slide b.
 */
#ifndef MOC_HIP_H
#define MOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOC_ABI_VERSION 20

enum { MOC_TICKET_QUEUES = 64, MOC_TICKET_STRIDE = 64,     /* moc_batch_t.tile_ticket: counters, int32 words between them */
       MOC_TICKET_WORDS = (64 + 8) * 64 };

enum { MOC_OK = 0, MOC_EINVAL = 1, MOC_EUNSUPPORTED = 2, MOC_ELAUNCH = 3 };

/* storage type of the bag X; arithmetic is always fp32-accumulate */
enum { MOC_F32 = 0, MOC_BF16 = 1, MOC_F16 = 2 };

/* moc_batch_t.flags.  MOC_STATS_COMPACT: the score pass writes C+5 statistics per row instead of 2C+3 -- the C softmax
 * columns (patch_selection_classifier_index.py:34) are not stored; their consumers (moc_select's psi_sigma keys,
 * moc_gather_candidates' s_sigma) re-form softmax[c] = exp2((logit[c] - m1) * log2 e) * (1/den) from the row maximum m1
 * and the reciprocal of the denominator, with the score pass's own arithmetic: the same bits.  For wide banks, where the
 * statistics are a quarter of the pass's HBM traffic (thirty classes: 253 -> 141 bytes per 1 KiB row).  moc_row_stats
 * and callers that read `stats` themselves (the zero-shot poolings) use the full layout. */
enum { MOC_STATS_COMPACT = 1,
       /* moc_select: one workgroup per column even for wide banks (the default there is one workgroup per slide and
        * group of eight columns); both give the same flags -- this bit exists so that tests can say so */
       MOC_SELECT_PER_COLUMN = 2,
       /* evaluation passes: moc_gather_candidates does not materialise the [2C+2, S] candidate columns of wide banks
        * (C > 4) and moc_meta_forward reads a selected row's four scores (main_moc.py:359-366, :482-492) straight from
        * `stats` through sel_idx -- the same values.  Entry points that need `cand` itself (the train steps,
        * moc_mix_fixed, moc_pack_selected*) refuse such a batch. */
       MOC_CAND_FROM_STATS = 4,
       /* moc_meta_forward over many slides: keep to 64 rows per workgroup (the default for launches of at least four
        * slides with 1024 or more selectable rows on 16-bit bags is 128 rows per workgroup, rows by LDS-DMA); both give
        * the bits of the one-slide kernel -- the bit exists so that tests can say so */
       MOC_FORWARD_ROWS64 = 8,
       /* moc_meta_forward on fp32 bags, 16 rows per workgroup: keep to four waves, every wave the whole chain over the
        * columns of its hidden units (the default splits the columns over four wave groups, sixteen waves: the training
        * step's forward); the same bits -- the bit exists so that tests can say so */
       MOC_FORWARD_FOUR_WAVES = 16,
       /* moc_meta_forward of ONE slide on 16-bit bags: keep to 16 rows per workgroup even when the slide has 16,384 or
        * more selectable rows (the default there is the 64-row kernel: every W1 fragment feeds four row tiles -- at
        * 25,000 rows the sixteen-row workgroups re-read 390 KB of W1 image 1,580 times); the same bits -- the bit exists
        * so that tests can say so */
       MOC_FORWARD_ROWS16 = 32,
       /* moc_scores / moc_scores_timed on fp32 bags against a bank of one n-tile (Ce <= 16): the LDS-DMA ring kernel
        * (one loader wave and three consumer waves per CU, rows through a ring of 16 KiB LDS slots, at most 64 VGPRs)
        * instead of the register-buffered streaming kernel, where its LDS fits; the same bits in every output.  Other
        * shapes keep their kernels.  The ring kernel walks the tiles statically over every CU: a batch that carries this
        * bit AND a tile_ticket or cu_reserved is refused.  moc_scores_form() says which form a batch gets. */
       MOC_SCORES_RING = 64 };

/* bits of `discard_bits`, in the order of main_moc.py:341-350 */
enum { MOC_SEL_TOPK = 1, MOC_SEL_DELTA_SOFTMAX = 2, MOC_SEL_DELTA_DIFF = 4, MOC_SEL_BOTTOMK = 8 };

typedef void* moc_stream_t; /* hipStream_t */

/* A batch of slides packed back to back in one [total_rows, D] array, plus the
 * caller-allocated work arrays every stage reads/writes.  `stride` below is
 * total_rows. */
typedef struct moc_batch {
    /* ---- inputs ---- */
    const void*    X;          /* device [total_rows, D]                                  */
    int32_t        dtype;      /* MOC_F32 | MOC_BF16 | MOC_F16 (storage; arithmetic is fp32) */
    int32_t        D;          /* embedding dim (512 for CONCH)                          */
    int64_t        total_rows;
    int32_t        n_slides;
    int32_t        max_rows;   /* host bound on the rows a slide brings to the selectors (sizes grids and picks kernel
                                  shapes): max rows of any slide, or -- tighter -- max KEPT rows (moc_host_max_kept) */
    const int64_t* row_off;    /* device [n_slides+1], first SLOT of each slide (prefix
                                  sum of the slide sizes)                                */
    const int64_t* row_off_host; /* host copy of row_off, or NULL.  With it, single-slide launches
                                  (the sequential train steps) get the slide's first slot as a
                                  kernel argument instead of a dependent device load          */
    const int64_t* x_off;      /* device [n_slides], first row of each slide inside X, or
                                  NULL = row_off (slides packed in batch order).  Lets a
                                  batch visit resident slides in any order / repeatedly
                                  (dataset_generic.py:380-393 repeat_num) without copies */
    const uint8_t* mask;       /* [total_rows] 0/1 keep flags in device OR device-mapped pinned host memory
                                  (read once, by moc_mask_compact), or NULL = keep all
                                  (main_moc.py:329-331; drawn by the host, see moc_amd)  */
    int32_t        C;          /* n_classes                                              */
    int32_t        Ce;         /* columns of zeroshot_weights_ext (C + background)       */
    int32_t        topj;       /* --topj                                                 */
    int32_t        topk;       /* --topk                                                 */
    uint32_t       discard_bits;
    uint32_t       flags;      /* MOC_STATS_COMPACT or 0 (the field was `reserved`, always 0, before round 3) */
    /* ---- work arrays (device) ---- */
    int32_t* kept;       /* [total_rows + 16] slot -> row index inside its slide (unused if mask==NULL);
                            the 16 entries of slack let the score pass read a tile's 16 indices
                            with one scalar load without running off the allocation            */
    int32_t* n_kept;     /* [n_slides]                                                               */
    float*   stats;      /* [2C+3, total_rows] per-slot: logits[C] | softmax[C] | gap | bg_sum | bg_max;
                            with MOC_STATS_COMPACT only the first C+5 rows are used:
                            logits[C] | m1 | 1/den | gap | bg_sum | bg_max                                 */
    uint8_t* sel_flag;   /* [total_rows]      union membership                                        */
    int32_t* sel_idx;    /* [total_rows]      selected_index of slide b at [row_off[b], +n_sel[b])     */
    int64_t* sel_row;    /* [total_rows]      same positions: row of X (packed) to gather             */
    int32_t* n_sel;      /* [n_slides]        S                                                       */
    float*   cand;       /* [2C+2, total_rows] per selected row: s_p[C] | s_sigma[C] | s_delta | s_beta */
    /* ---- placement of the score pass (round 3; both nullable = static walk over the whole chip) ---- */
    const uint32_t* cu_reserved; /* device [128]: compute units the score pass stays off (see moc_cu_census)   */
    int32_t*        tile_ticket; /* device [MOC_TICKET_WORDS]: the score pass's tile counters                  */
    /* ---- round 4, second session (nullable) ---- */
    const int32_t*  n_sel_host;  /* HOST [n_slides]: a copy of n_sel that the caller has seen arrive (e.g. an asynchronous
                                    copy behind phase A whose event has completed), or NULL.  The train steps then take
                                    a slide's S as a kernel argument instead of loading it -- one dependent round trip
                                    less at the head of the forward (arguments -> sel_row -> rows), exact grids, fewer
                                    record keys per lane in the step.  The same results either way.  Ignored by
                                    moc_train_steps_graph: a captured pass serves later passes too, with other counts.  */
    /* ---- the selected-row counts by mailbox (both nullable / 0; appended: a caller that zero-fills THIS struct is
     * served as before.  The struct grew by 16 bytes and the library reads them, so callers are rebuilt against this
     * header; the version number stays 20) ----
     * The asynchronous copy above tells the host every count of a pass at once, and only when the whole of phase A and
     * the copy behind it have run.  compact_kernel -- one workgroup per slide -- knows S long before: when n_sel_mail is
     * set, its thread 0 stores ((uint64_t)n_sel_ticket << 32) | (uint32_t)S to n_sel_mail[b] beside n_sel[b], as ONE
     * 64-bit system-scope store: count and ticket travel in one naturally aligned word, so no fence, counter or further
     * launch is needed.  Slide b's word is valid exactly when its upper half equals the ticket the caller expects; the
     * caller takes a fresh ticket for every launch that rewrites n_sel, so a word of an earlier phase A never passes.
     * moc_phase_a and moc_gather_candidates write the words; moc_train_steps reads slide b's word ONCE, in front of
     * step b's two launches (n_sel_host, when set, wins), and hands the count to both by value: a slide whose word has
     * not arrived runs on the device count.  The only wait is a bounded one in front of a call's FIRST step, for that
     * slide's word (MOC_N_SEL_SPIN_US microseconds at the most, default 100; 0: none): the words of a phase A arrive
     * together, at its end.  The same results either way.  moc_train_steps_graph
     * ignores both fields; the data-parallel, p2p and batched-run entries read n_sel_host only. */
    uint64_t*       n_sel_mail;   /* HOST [n_slides], device-mapped pinned (hipHostMalloc / a pinned tensor), 8-byte
                                     aligned; lives while launches that write it can be in flight */
    uint32_t        n_sel_ticket; /* the ticket the caller expects in the words' upper halves; 0: none */
} moc_batch_t;

/* The meta-learner ("senet", main_moc.py:299-312) and its Adam state
 * (main_moc.py:316; torch.optim.Adam defaults otherwise).  All device fp32. */
typedef struct moc_meta {
    float *W1, *b1, *W2, *b2;         /* [H,D] [H] [4,H] [4]   H = 64                      */
    float *m_W1, *m_b1, *m_W2, *m_b2; /* exp_avg      (may be NULL for forward-only use)   */
    float *v_W1, *v_b1, *v_W2, *v_b2; /* exp_avg_sq                                        */
    float *g_W1, *g_b1, *g_W2, *g_b2; /* gradient outputs (moc_train_grad), may be NULL    */
    void  *W1_image;                  /* device scratch, moc_w1_image_bytes(D, dtype): W1 re-laid in
                                         MFMA operand order for the forward pass, three 16-bit terms
                                         per weight for every storage (ABI 19).  Derived data the
                                         library rebuilds / keeps in sync itself; contents need not
                                         survive between calls.
                                         RANGE, fp16 bags only: the fp16 image holds the three fp16 terms
                                         of w * 2^10, so every |W1[i]| must stay below 32 (beyond 64 the
                                         high term overflows fp16).  This is the CALLER's contract: the
                                         library does not check it -- the step kernels rewrite W1 and its
                                         image on the device, and a check would cost a host round trip
                                         per step.  nn.Linear starts at |w| <= 1/sqrt(D); a caller whose
                                         weights can grow that far keeps its bags in bf16 or fp32, whose
                                         images have fp32's exponent range (no such limit).  The
                                         classifier bank's fp16 limit, |w| < 2, IS checked
                                         (moc_prepare_bank).                                    */
    double lr, beta1, beta2, eps, weight_decay; /* the optimizer's Python floats, unrounded     */
    int32_t H;                        /* hidden width, must be 64                          */
    int32_t D;                        /* input width (== batch D)                          */
    int64_t step;                     /* Adam steps already taken                          */
} moc_meta_t;

/* Work arrays of the meta-learner stage, caller allocated (device). */
typedef struct moc_meta_ws {
    float*   H1;        /* [total_rows, H]  relu(W1 x + b1) of every selected row            */
    float*   gates;     /* [total_rows, 4]  lambda                                           */
    float*   mixed;     /* [C, total_rows]  gated sum of the candidates ("final_logits")     */
    float*   pooled;    /* [n_slides, C]    top-K mean per class                             */
    int32_t* topk_idx;  /* [n_slides, C, topk] positions (0..S) of the pooled rows, by value */
    int32_t* topk_cnt;  /* [n_slides, C]    min(K, S)                                        */
    float*   loss;      /* [n_slides]       cross entropy                                    */
    int32_t* pred;      /* [n_slides]       argmax of pooled                                 */
    float*   pair_dh;   /* [C*topk, H]      backward scratch (one slide at a time)           */
    float*   W2_alt;    /* [4, H]           second copy of W2: the one-launch step reads one and writes
                                            the other (may be NULL: three-launch step is used)      */
    int64_t* pair_row;  /* [C*topk]                                                          */
    int32_t* n_pair;    /* [1]                                                               */
    /* round 4: tile records (nullable).  Scratch of moc_tile_ws_bytes(total_rows, n_slides, C) bytes, 16-byte aligned:
     * the forward of a training step leaves, per 16-row tile and class, the tile's four largest mixed scores with
     * their rows' ids, gates and candidate scores; the one-launch step then pools among those records instead of
     * re-reading and ranking every mixed score (exactness checked in the kernel, full scores as the fall-back).
     * NULL: the round-3 step. */
    void*    tile_ws;
    int64_t  tile_ws_bytes;
} moc_meta_ws_t;

int         moc_version(void);
const char* moc_last_error(void);
size_t      moc_w1_image_bytes(int D, int dtype);
size_t      moc_tile_ws_bytes(int64_t total_rows, int n_slides, int C);   /* moc_meta_ws_t.tile_ws */

/* ---- classifier bank ------------------------------------------------------
 * Re-lays [zeroshot_weights | zeroshot_weights_ext[:, C:]] (main_moc.py:336-337:
 * the foreground columns come from W, the background ones from W_ext) into the
 * MFMA operand image the score kernel streams from LDS.  For MOC_BF16 bags the
 * fp32 weights are split into three bf16 terms so products stay exact in fp32.
 * Redo whenever the weights change.  `fg_from_ext` != 0 takes the foreground
 * columns from W_ext[:, :C] instead (bottomk_irrel_classifier_pooling,
 * utils/patch_selection_classifier.py:151). */
size_t moc_bank_bytes(int D, int Ce, int dtype);
int    moc_prepare_bank(const float* W /*device [D,C]*/, const float* W_ext /*device [D,Ce]*/,
                        int D, int C, int Ce, int dtype, int fg_from_ext,
                        void* bank_out /*device, moc_bank_bytes*/, moc_stream_t stream);

/* ---- phase A: parameter-free part of slide_process (main_moc.py:322-366) ---- */

/* a1  row mask -> kept list + n_kept (main_moc.py:329-331).  No-op when mask==NULL. */
int moc_mask_compact(const moc_batch_t* B, moc_stream_t stream);

/* a1, host side: the row masks of `n` consecutive rows exactly as main_moc.py:330 draws them
 * (`torch.rand(N) > 0.5`, CPU default generator = mt19937, one output per sample).  rng_state is
 * the byte image of torch.get_rng_state() (in/out: advanced by n draws, hand it back with
 * torch.set_rng_state); out gets n 0/1 bytes.  Returns the number of kept rows, -1 on error.
 * Pure host code: same bits as torch.rand, no GPU involved. */
int64_t moc_host_draw_masks(uint8_t* rng_state, int64_t state_bytes, int64_t n, uint8_t* out);

/* Largest number of non-zero flags of any slide, `mask` being the host keep flags of a batch laid out by
 * row_off_host[n_slides + 1]: a tight `max_rows` for a masked batch (the selectors only ever see the kept rows of
 * `feat[mask]`, main_moc.py:329-331), which lets wide shapes pool inside the step kernel.  Host only; -1 on bad
 * arguments. */
int64_t moc_host_max_kept(const uint8_t* mask, const int64_t* row_off_host, int n_slides);

/* a2 + per-row parts of a4-a6, a9: X.[W|W_ext] and the row statistics
 * (main_moc.py:336-337, :360-365; patch_selection_classifier_index.py:34, :46-48, :75).
 * Also clears sel_flag. */
int moc_scores(const moc_batch_t* B, const void* bank, moc_stream_t stream);
/* moc_scores with two hipEvent_t (created with timing enabled) that receive the score kernel's own start and end
 * time stamps (hipExtLaunchKernel): hipEventElapsedTime(start, stop) is then the kernel's duration as a profiler
 * reports it, whatever else the GPU is running.  bench.py's `roofline` uses it. */
int moc_scores_timed(const moc_batch_t* B, const void* bank, moc_stream_t stream, void* start_event, void* stop_event);
/* Which kernel form moc_scores gives this batch (no launch): 0 streaming, 1 wide ring, 2 wide, 3 generic, 4 the LDS-DMA
 * ring of MOC_SCORES_RING; negative: the batch is refused (moc_last_error has the text moc_scores would give). */
int moc_scores_form(const moc_batch_t* B);

/* a2 for several NARROW banks in one read of the bags (additive in ABI 20): prompt-bank selection.  A bank of at most 16
 * columns is one n-tile of the score kernel's image; up to moc_scores_banks_max of them laid side by side are an image its
 * main loop multiplies as it is, and a per-n-tile row epilogue writes bank g's statistics into bank g's own arrays -- bit
 * for bit what moc_scores writes over a batch with that bank alone (a column's accumulation chain does not depend on which
 * other columns share the MFMA; the epilogue is the one-n-tile epilogue on the bank's own window of the tile).
 * From B the entry takes X, dtype, D, the slide layout (row_off, x_off, total_rows, n_slides, max_rows) and the mask lists
 * (mask, kept, n_kept: run moc_mask_compact first); B->stats, B->sel_flag, B->C, B->Ce, B->topj and B->topk are ignored.
 * An evaluation pass: static walk over the whole chip, full statistics layout -- a batch with tile_ticket / cu_reserved
 * set or with MOC_STATS_COMPACT is refused (MOC_EINVAL), as are a null pointer, n_banks outside 1 .. 4, a Ce outside
 * C < Ce <= 16 and more banks than moc_scores_banks_max; MOC_EUNSUPPORTED where not even one bank's image fits in LDS
 * beside the epilogue tiles and one slide's metadata (moc_scores_banks_max == 0).  Nothing is launched on a refusal.
 * stats[g] / sel_flag[g] are only ever addressed as stats[g] + r * B->total_rows + row_off[b] + i and sel_flag[g] +
 * row_off[b] + i with 4- and 1-byte stores: they need only 4- / 1-byte alignment and may lie INSIDE a larger array of the
 * same row stride -- a batch's own stats / sel_flag advanced by a number of slots, which lands bank g's statistics of
 * slide b in the slots of another slide of the same size (moc_amd/runs.py: training under several banks). */
int    moc_scores_banks_max(int D, int dtype);             /* banks one launch serves for this D / storage: the streaming
                                                              kernel's n-tile limits (four on fp32 bags, three on 16-bit
                                                              bags) and 160 KiB of LDS; 0 = none */
size_t moc_bank_set_bytes(int D, int n_banks, int dtype);  /* n_banks one-n-tile images back to back */
typedef struct moc_bank_set {
    int32_t  n_banks;            /* 1 .. moc_scores_banks_max */
    int32_t  C;                  /* the same for every bank */
    int32_t  Ce[4];              /* per bank, C < Ce <= 16 */
    float*   stats[4];           /* per bank [2C+3, B->total_rows], full layout */
    uint8_t* sel_flag[4];        /* per bank [B->total_rows], cleared by the pass as moc_scores does */
    const void* image;           /* moc_bank_set_bytes: bank g's image (moc_prepare_bank with its own Ce, fg_from_ext) at
                                    g * moc_bank_bytes(D, 16, dtype) */
} moc_bank_set_t;
int moc_scores_banks(const moc_batch_t* B, const moc_bank_set_t* S, moc_stream_t stream);

/* a2 from a cache (round 4, opt-in): the statistics of a row depend only on the row and the frozen bank, so a resident
 * split can keep the statistics of ALL its rows (`stats_all` [rows of stats, all_rows], laid out like `stats` and indexed
 * by the row's position in B->X: the output of an UNMASKED moc_scores over the split with the same B->flags layout) and a
 * pass then copies the kept rows' statistics into slot order instead of reading the bags again (main_moc.py:336-337 is
 * recomputed per visit in the reference; the bits are the same).  Needs moc_mask_compact's lists for a masked batch. */
int moc_scores_from_cache(const moc_batch_t* B, const float* stats_all, int64_t all_rows, moc_stream_t stream);

/* The same statistics from an already computed logits matrix (device [N, Ct] row-major,
 * first C columns foreground): stats_out is [2C+3, N].  For callers that hold logits, not
 * bags (index_*_classifier / *_pooling, utils/patch_selection_classifier*.py).  With C == 1
 * the gap column is +inf (the reference's topk(2) would raise). */
int moc_row_stats(const float* logits, int64_t N, int Ct, int C, float* stats_out, moc_stream_t stream);

/* a3-a7: the four top-j selectors and their union, as flags
 * (patch_selection_classifier_index.py:17-87, main_moc.py:341-352). */
int moc_select(const moc_batch_t* B, moc_stream_t stream);

/* a7-a9: ascending compaction of the union -> sel_idx/sel_row/n_sel, candidate
 * scores of the selected rows, optionally the gathered rows themselves
 * (main_moc.py:354-366).  selected_feat: device [total_rows, D] in X's dtype or NULL. */
int moc_gather_candidates(const moc_batch_t* B, void* selected_feat, moc_stream_t stream);

/* all four above, in order */
int moc_phase_a(const moc_batch_t* B, const void* bank, moc_stream_t stream);

/* ---- hyper-parameter grids: one score pass for the slides that visit the same rows under the same mask ----------
 * Runs that differ only in topj / topk / discard_bits see the same kept rows and the same statistics (everything in front of
 * moc_select depends on none of the three).  After moc_mask_compact + moc_scores (or moc_scores_from_cache) over the LEADER
 * slides, every follower slide b in [slide0, slide0 + n) with leader l = leader_of_slide[b] (device int32 [B->n_slides],
 * indexed by the slide's position in the batch; a negative value: b is not a follower and is left alone) receives
 *   n_kept[b] = n_kept[l];   kept[row_off[b] + i] = kept[row_off[l] + i];
 *   stats[r][row_off[b] + i] = stats[r][row_off[l] + i]  for every row r of the layout B->flags names (2C+3, or C+5 with
 *   MOC_STATS_COMPACT);   sel_flag[row_off[b] + i] = 0 (as the score pass leaves it)            for i < n_kept[l]
 * -- everything moc_select / moc_gather_candidates read per slot; the follower then is, bit for bit, a slide the score pass
 * ran over.  An unmasked batch copies the statistics of all rows of l.  A leader may lie behind its follower and may have
 * several; a leader must not itself be a follower.  l is CLAMPED into the batch on the device and the copy never leaves
 * either slide's slots (a follower and its leader are meant to have equal sizes): nothing outside the arrays is touched.
 * Errors (not faults), before anything is launched: null B / leader_of_slide, a batch without stats / sel_flag, a bad slide
 * range.  Additive to ABI 20: the version number is unchanged. */
int moc_stats_share(const moc_batch_t* B, const int32_t* leader_of_slide, int slide0, int n, moc_stream_t stream);

/* The lists-only half of moc_stats_share (additive to ABI 20): for followers whose statistics their OWN score pass writes --
 * runs that train under another prompt bank see their leader's masks and none of its scores.  Every follower slide b in
 * [slide0, slide0 + n) with leader l = leader_of_slide[b] (as above: device int32 [B->n_slides], negative = left alone,
 * clamped into the batch on the device) receives
 *   n_kept[b] = n_kept[l];   kept[row_off[b] + i] = kept[row_off[l] + i]   for i < n_kept[l]
 * with the count clamped to both slides' sizes.  stats and sel_flag are NOT touched (they may be null): the pass that scores
 * the follower's slots writes the statistics and clears the flags.  An unmasked batch has no lists: MOC_OK, nothing launched.
 * Errors (not faults), before anything is launched: null B / leader_of_slide, a masked batch without kept / n_kept, a bad
 * slide range. */
int moc_kept_share(const moc_batch_t* B, const int32_t* leader_of_slide, int slide0, int n, moc_stream_t stream);

/* Phase A's result for slides [slide0, slide0+n) in a fixed-capacity, position-independent form -- what
 * slide_process hands to the meta-learner (main_moc.py:367-375: selected_feat + the four candidate matrices),
 * `cap` rows per slide: feat_out device [n][cap][D] in X's dtype, cand_out device [n][2C+2][cap] fp32; entries at
 * and beyond n_sel[slide] are not written.  The exact-sequential multi-GPU mode (SURVEY.md section 8e mode 1)
 * all-gathers these blocks so that every GPU runs the reference's one-Adam-step-per-slide recurrence
 * (main_moc.py:380-410) over slides whose phase A ran elsewhere. */
int moc_pack_selected(const moc_batch_t* B, int slide0, int n, int cap, void* feat_out, float* cand_out,
                      moc_stream_t stream);

/* The same hand-over without padding, for a gather of unequal pieces: slide slide0+b's min(n_sel, cap) rows start at
 * row sum_{q<b} min(n_sel[slide0+q], cap) of feat_out (device [out_rows][D], X's dtype), and its candidate scores are
 * the rows cand_out[that row + t][2C+2] (device fp32, ROW-major: s_p[C] | s_sigma[C] | s_delta | s_beta per selected
 * row -- main_moc.py:359-366's four matrices side by side); rows at and beyond out_rows are dropped.  What the
 * exact-sequential mode sends since round 3: sum S rows per rank instead of n x cap (44 % less at NSCLC-16). */
int moc_pack_selected_rows(const moc_batch_t* B, int slide0, int n, int cap, void* feat_out, float* cand_out,
                           int64_t out_rows, moc_stream_t stream);

/* ---- phase B: meta-learner, pooling, loss, update ------------------------- */

/* use_bits: which of the four gated terms enter the sum (bit i = term i).
 * train: ~discard_bits & 15 (main_moc.py:396-403); eval: see moc_amd.main_moc
 * for the reference's quirk (main_moc.py:486-492). */

/* a10-a11 for slides [slide0, slide0+n): H1, gates, mixed.  ws->H1 / ws->gates may be NULL (evaluation:
 * only the backward pass reads them; 256 + 16 bytes per selected row not written). */
int moc_meta_forward(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                     int slide0, int n, uint32_t use_bits, moc_stream_t stream);

/* Patch maps (ABI 20): every row of slides [slide0, slide0 + n) of an UNMASKED batch whose score pass has run (moc_scores
 * or moc_phase_a, either statistics layout) gets what moc_meta_forward gives a selected row -- its gates and gated mix, bit
 * for bit -- without the sel_row gather: row i of slide b is X row x_off[b] + i (row_off[b] + i without x_off), its slot
 * row_off[b] + i, its candidate scores the statistics at that slot.  gates: device [total_rows, 4] or NULL; mixed: device
 * [C, total_rows]; both indexed by slot like moc_meta_ws_t and written only at the slots of the n slides (the caller's
 * buffers: an evaluation's ws->mixed, which moc_pool_loss reads, is left alone).  Error (not a fault) if B->mask != NULL
 * or B->stats is unset.  use_bits as for moc_meta_forward. */
int moc_meta_forward_dense(const moc_batch_t* B, const moc_meta_t* M, float* gates, float* mixed,
                           int slide0, int n, uint32_t use_bits, moc_stream_t stream);

/* ablation_evaluation's parameter-free mixes (main_moc.py:538-553) in place of
 * moc_meta_forward: mode 0 = avg (0.25 each), 1 = sum, 2 = max of the four candidates. */
int moc_mix_fixed(const moc_batch_t* B, const moc_meta_ws_t* ws, int slide0, int n, int mode,
                  moc_stream_t stream);

/* a12-a13 (+a16 argmax) for slides [slide0, slide0+n): pooled, topk_idx, loss, pred.
 * labels: device int64 [n_slides]. */
int moc_pool_loss(const moc_batch_t* B, const moc_meta_ws_t* ws, const int64_t* labels,
                  int slide0, int n, moc_stream_t stream);

/* a13 + a16 alone: cross entropy and argmax of n rows of pooled logits [n, C]
 * (F.cross_entropy(logits, lbl) and logits.argmax(dim=1), main_moc.py:433-434, :494-495). */
int moc_ce_loss(const float* pooled, const int64_t* labels, int n, int C, float* loss, int32_t* pred,
                moc_stream_t stream);

/* Batched runs (round 4): `n_runs` independent meta-learners stepped in lockstep by ONE forward launch and ONE step launch
 * per meta-step (grid.y / grid.z = run) -- the folds x shots of the reference's launcher (scripts/moc_train.sh:11-31) as
 * one process per GPU instead of one process per run.  Run r owns the slides slide0 + r * slide_stride ... of B, its tensors
 * lie par_stride floats behind run 0's in ONE arena per kind (W1 | b1 | W2 | b2 of a run inside one block, the moments
 * laid out alike), its W1 operand image image_stride bytes behind run 0's.  All runs share the Adam hyper-parameters and
 * step count of M.  Per run the arithmetic is moc_train_steps's: bit-identical parameters. */
typedef struct moc_runs {
    int32_t n_runs;        /* 1 .. 16 */
    int32_t slide_stride;  /* slides of B between consecutive runs' first slides (>= n) */
    int64_t par_stride;    /* floats */
    int64_t image_stride;  /* bytes, >= moc_w1_image_bytes(D, dtype) */
} moc_runs_t;
/* M: run 0's tensors.  ws->W2_alt: [n_runs, 4, H].  With ws->tile_ws and a shape of the tile-record step (C <= 16, K <= 16,
 * C K <= 64, <= 4,096 selectable rows) the runs step in lockstep (moc_train_runs_mode == 1); other shapes of the one-launch
 * steps (wide banks: EBRAINS-30, the 64-way shape) take every run's pass one after the other on `stream`, with the launches
 * of moc_train_steps (mode 2: give every run a call and a stream of its own to have their chains side by side); shapes of
 * the three-launch step are refused (mode 0: its scratch is one per batch). */
int moc_train_steps_runs(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                         const int64_t* labels, int slide0, int n, uint32_t use_bits, moc_stream_t stream);
int moc_train_runs_mode(const moc_batch_t* B, const moc_meta_ws_t* ws);

/* Batched runs with Adam hyper-parameters PER RUN (ABI 20, additive): moc_train_steps_runs, except that run r is updated
 * with hp[r] instead of M's lr / betas / eps / weight_decay -- a seeds x lr x weight-decay grid whose cells share a split
 * and a mask stream and differ in the last instructions of the step.  hp: HOST array of R->n_runs records, read before
 * the call returns; the values are the optimizers' unrounded Python floats, as in moc_meta_t.  The step count is still
 * M->step for every run.  In lockstep shapes (moc_train_runs_mode == 1) the coefficients of run r at every step are formed
 * on the host with the arithmetic of moc_train_steps (doubles, rounded to fp32 once) and travel in the step launch's
 * argument block, up to eight runs per step launch (more runs: two step launches behind the one forward launch); in
 * mode 2 every run's pass takes its record in place of M's values.  Per run bit-identical to moc_train_steps with a
 * moc_meta_t that holds hp[r].  Errors (not faults), before anything is launched: everything moc_train_steps_runs
 * refuses, a null hp, a non-finite or negative lr / eps / weight_decay, a beta outside [0, 1). */
typedef struct moc_adam_hp {
    double lr, beta1, beta2, eps, weight_decay;
} moc_adam_hp_t;
int moc_train_steps_runs_hp(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                            const int64_t* labels, int slide0, int n, uint32_t use_bits, const moc_adam_hp_t* hp,
                            moc_stream_t stream);

/* Prediction with several meta-learners (an ensemble of checkpoints; ABI 20, additive): the evaluation forward of
 * moc_meta_forward for R->n_runs models (1 .. 16) over the union rows of slides [slide0, slide0 + n) of an UNMASKED batch
 * whose phase A has run, in one launch: the row ids and candidate scores are read once per tile for all models.  Model r's
 * parameters lie r * R->par_stride floats behind M's (W1 | b1 | W2 | b2 of a model in one block, as moc_train_steps_runs
 * lays them out), its W1 image r * R->image_stride bytes behind M->W1_image (rebuilt here for every model).
 * R->slide_stride must be 0: every model works on the same slides.  mixed: device [n_runs][C][total_rows] fp32, model r's
 * slab indexed by slot like moc_meta_ws_t.mixed and written at the union slots of the n slides -- bit for bit what
 * moc_meta_forward gives with model r alone (pool each slab with moc_pool_loss through a ws whose `mixed` points at it).
 * Errors (not faults), before anything is launched: a masked batch, no phase-A outputs, null mixed, n_runs outside
 * 1 .. 16, nonzero slide_stride, par_stride / image_stride smaller than one model.  use_bits as for moc_meta_forward. */
int moc_meta_forward_models(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, float* mixed,
                            int slide0, int n, uint32_t use_bits, moc_stream_t stream);

/* Evaluation of several runs in one pass (ABI 20, additive): the evaluation forward of moc_meta_forward over the union rows
 * of slides [slide0, slide0 + n) of an UNMASKED batch whose phase A has run, in ONE launch, in which every slide names the
 * meta-learner that scores it: slide b is scored by model model_of_slide[b] (device int32 [B->n_slides], indexed by the
 * slide's position in the batch, values 0 .. R->n_runs - 1).  Model r's parameters lie r * R->par_stride floats behind M's,
 * its W1 image r * R->image_stride bytes behind M->W1_image (the arena layout of moc_train_steps_runs and
 * moc_meta_forward_models; the images of all n_runs models are rebuilt here).  R->slide_stride must be 0.  ws->mixed is
 * written at the union slots of the n slides exactly as moc_meta_forward writes it (ws->H1 / ws->gates too when they are not
 * NULL), so one moc_pool_loss then pools all slides: for a slide of model r the mixed scores are, bit for bit, what
 * moc_meta_forward gives with model r alone.  Always the 128-row evaluation kernel, whatever the shape (the smaller
 * evaluation kernels give the same bits).  An index outside 0 .. n_runs - 1 is CLAMPED into that range on the device (the
 * slide is then scored by model 0 or n_runs - 1): nothing is read outside the arenas.
 * Errors (not faults), before anything is launched: a masked batch, no phase-A outputs, null model_of_slide, null ws or
 * ws->mixed, n_runs outside 1 .. 16, nonzero slide_stride, par_stride / image_stride smaller than one model, meta D != batch
 * D, a bad slide range.  use_bits as for moc_meta_forward. */
int moc_meta_forward_by_slide(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R,
                              const int32_t* model_of_slide, const moc_meta_ws_t* ws, int slide0, int n, uint32_t use_bits,
                              moc_stream_t stream);

/* Ensemble patch maps (ABI 20, additive): the dense forward of moc_meta_forward_dense for R->n_runs models (1 .. 16) over
 * EVERY row of slides [slide0, slide0 + n) of an UNMASKED batch whose score pass has run, the models reduced on the device.
 * With p_r = softmax_c(scale * mixed_r) of model r alone (scale: the evaluation temperature, 56.3477):
 *   prob_mean  [C][total_rows]  (1/R) sum_r p_r                        required
 *   prob_std   [C][total_rows]  sqrt((1/R) sum_r (p_r - mean)^2)       (population std; may be NULL)
 *   gates_mean [total_rows][4]  (1/R) sum_r gates_r                    (may be NULL)
 * indexed by slot like moc_meta_forward_dense's outputs and written at the rows of the n slides only.  fp32, in model order
 * (a Welford update): the same inputs give the same bits.  The per-model slabs never reach memory.  Parameters and W1 images
 * as for moc_meta_forward_models (par_stride / image_stride; the images are rebuilt here), R->slide_stride must be 0.
 * Errors (not faults), before anything is launched: a masked batch, no statistics, null prob_mean, n_runs outside 1 .. 16,
 * nonzero slide_stride, par_stride / image_stride smaller than one model, meta D != batch D, C > 64, a bad slide range,
 * a scale that is not finite.  use_bits as for moc_meta_forward. */
int moc_meta_forward_dense_models(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, float scale,
                                  float* prob_mean, float* prob_std, float* gates_mean, int slide0, int n, uint32_t use_bits,
                                  moc_stream_t stream);

/* a10-a14 for ONE slide without the update: forward, pooling, loss (ws->loss/pooled/pred) and
 * the gradients of that loss w.r.t. the four parameter tensors, written (not accumulated) to
 * M->g_*.  The data-parallel step all-reduces them and calls moc_adam_step. */
int moc_train_grad(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                   const int64_t* labels, int slide, uint32_t use_bits, moc_stream_t stream);

/* a14 for a caller-written loop (main_moc.py:390-410 kept as it is around slide_process): the backward of
 * `lambdas = model(selected_feat)` given d loss / d lambdas.  X [S, D] are the rows the forward ran on (storage `dtype`),
 * H1 [S, H] / gates [S, 4] what moc_meta_forward left for them, grad_gates [S, 4] autograd's gradient (rows of zeros
 * carry nothing and are skipped).  Writes (does not accumulate) g_W1 [H, D], g_b1 [H], g_W2 [4, H], g_b2 [4].
 * Scratch, all device: pair_dz [S, 4], pair_dh [S, H], pair_row [S], n_pair [1]. */
int moc_senet_backward(const void* X, int dtype, int64_t S, int D, const float* H1, const float* gates,
                       const float* grad_gates, const float* W2, float* g_W1, float* g_b1, float* g_W2, float* g_b2,
                       float* pair_dz, float* pair_dh, int64_t* pair_row, int32_t* n_pair, moc_stream_t stream);

/* a15: one Adam step (coupled L2) from M->g_* scaled by grad_scale; uses step = M->step+1. */
int moc_adam_step(const moc_meta_t* M, float grad_scale, moc_stream_t stream);

/* e (data-parallel training): `n` synchronous steps on THIS rank's slides slide0..slide0+n-1.
 * Per step: forward, pooling, loss and gradients (as moc_train_grad), ONE all-reduce of the
 * flat gradient, the Adam step with grad_scale = 1/world (as moc_adam_step, step = M->step+1+t).
 * The collective is the caller's: `allreduce` has ncclAllReduce's signature (RCCL is not linked
 * into this library) and is called as allreduce(grad_flat, grad_flat, grad_count, ncclFloat32,
 * ncclSum, comm, stream); M->g_* must point into grad_flat.  NULL allreduce with world == 1
 * runs the same step sequence without a collective.  M->step itself is not advanced. */
typedef int (*moc_allreduce_fn)(const void* sendbuf, void* recvbuf, size_t count, int datatype, int op,
                                void* comm, moc_stream_t stream);
int moc_train_steps_dp(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                       const int64_t* labels, int slide0, int n, uint32_t use_bits,
                       float* grad_flat, int64_t grad_count, moc_allreduce_fn allreduce,
                       void* comm, int world, moc_stream_t stream);

/* e, one node: the same synchronous step with the exchange INSIDE the step kernel.  Every rank
 * writes its gradient straight into its peers' receive buffers over xGMI (IPC-mapped, fine-grained
 * memory), flags them, and sums the slices in rank order before its Adam update: two launches per
 * step instead of three plus a collective, bit-identical parameters on every rank.
 *   moc_p2p_create   allocate this rank's receive buffer for n_par = 64*D + 324 floats (current device)
 *   moc_p2p_export   write moc_p2p_handle_bytes() bytes the peers need (exchange them out of band,
 *                    e.g. torch.distributed.all_gather_object)
 *   moc_p2p_connect  `blobs` = the world's exports concatenated in rank order
 *   moc_p2p_allreduce  stand-alone sum of buf[0..n) over the ranks (self-check / small vectors)
 *   moc_p2p_error    0, or 1 + the rank that stayed silent past the time-out (5 s; MOC_P2P_TIMEOUT_MS)
 * Every rank must issue the same sequence of exchanges.  Ranks must be on one node, world <= 8. */
typedef struct moc_p2p moc_p2p_t;
int moc_p2p_handle_bytes(void);
int moc_p2p_create(int world, int rank, int64_t n_par, moc_p2p_t** out);
int moc_p2p_export(moc_p2p_t* comm, void* blob);
int moc_p2p_connect(moc_p2p_t* comm, const void* blobs);
int moc_p2p_allreduce(moc_p2p_t* comm, float* buf, int64_t n, moc_stream_t stream);
int moc_p2p_error(moc_p2p_t* comm);
int moc_p2p_destroy(moc_p2p_t* comm);
/* 1 when moc_train_steps_p2p handles these run constants (a function of them alone, so that every
 * rank takes the same decision whatever its bag sizes) */
int moc_p2p_step_supported(int C, int topk, int D, int topj);
int moc_train_steps_p2p(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                        const int64_t* labels, int slide0, int n, uint32_t use_bits,
                        moc_p2p_t* comm, moc_stream_t stream);

/* f4: gated-attention MIL pooling, the aggregation of the ABMIL / CLAM baselines
 * (models/model_clam.py:41-64 Attn_Net_Gated; :178-183, :206 CLAM_SB; :291-296, :318 CLAM_MB):
 *   a = tanh(h Wa^T + ba), b = sigmoid(h Wb^T + bb)        [N, D]   (nn.Linear layout: Wa, Wb are [D, L])
 *   A_raw[k][n] = Wc[k] . (a[n] * b[n]) + bc[k]             [K, N]   -- written (the reference returns it)
 *   M[k] = sum_n softmax_n(A_raw[k])[n] * h[n]              [K, L]
 * h: device fp32 [N, L] row-major, 16-byte aligned; L % 16 == 0; D in {128, 256, 384}; K <= 64.
 * workspace: moc_gated_attention_workspace(N, L, D, K) bytes of device memory, 16-byte aligned. */
size_t moc_gated_attention_workspace(int64_t N, int L, int D, int K);
int moc_gated_attention_pool(const float* h, int64_t N, int L, const float* Wa, const float* ba,
                             const float* Wb, const float* bb, int D, const float* Wc, const float* bc,
                             int K, float* A_raw, float* M, void* workspace, size_t workspace_bytes,
                             moc_stream_t stream);

/* The backward of moc_gated_attention_pool (what autograd does behind Attn_Net_Gated.forward + softmax + mm:
 * models/model_clam.py:58-63, :178-183, :206; the CLAM trainer calls loss.backward(), utils/core_utils.py:291).
 * Given gA [K, N] (gradient at A_raw; nullable) and gM [K, L] (gradient at M; nullable; 16-byte aligned), one
 * recompute pass over the bag (the forward's main loop: no activations were kept) writes
 *   dab [N, S]        S = moc_gated_attention_dab_stride(D, K) = 2 D + 16 ceil(K / 16): columns [0, D) and [D, 2 D)
 *                     the gradients at the two pre-activations h Wa^T + ba | h Wb^T + bb; column 2 D + k the
 *                     softmax p[k][n] = softmax_n(A_raw[k]); the rest zero
 *   ds  [K, N]        total gradient at A_raw: p (dp - sum_n p dp) + gA with dp[k][n] = h[n] . gM[k]
 *   dcol[(2 + K) D]   d_ba [D] | d_bb [D] | d_Wc [K, D]
 *   dbc [K]           d_bc
 * (every sum in a fixed order: deterministic).  What remains are two plain GEMMs the caller hands to a library
 * (rocBLAS / hipBLASLt: torch.mm) over X = [Wa; Wb; gM; 0] ([S, L]; zeros for gM when it is null):
 *   dh = dab X      and      dab^T h = [dWa; dWb; (M, unused)].
 * Same shape limits as the forward; workspace: moc_gated_attention_backward_workspace bytes, 16-byte aligned. */
size_t moc_gated_attention_backward_workspace(int64_t N, int L, int D, int K);
int moc_gated_attention_dab_stride(int D, int K);
int moc_gated_attention_backward(const float* h, int64_t N, int L, const float* Wa, const float* ba,
                                 const float* Wb, const float* bb, int D, const float* Wc, int K,
                                 const float* A_raw, const float* gA /*nullable*/, const float* gM /*nullable*/,
                                 float* dab, float* ds, float* dcol, float* dbc, void* workspace,
                                 size_t workspace_bytes, moc_stream_t stream);

/* f3: the per-patch logits of the adapter heads, one pass over the bag
 * (models/model_adapters.py:185-193 Conch_CLIP_Ada.forward; :330-405 Conch_MOE_CLIP_Ada.forward with the soft router,
 * use_switch_gate=False) -- everything in front of the top-j pooling.  unit(v) = v / ||v|| (a zero row gives NaN):
 *   E == 1:  a = relu(W2 relu(W1 x));  logits = unit(ratio a + (1 - ratio) x) Wc
 *   E >= 2:  f = unit(x);  w = softmax_E(G f);  a_e = relu(W2_e relu(W1_e f));  s = unit(sum_e w_e a_e);
 *            logits = unit(ratio s + (1 - ratio) f) Wc       (ratio is the module's stored clip_ratio / E)
 * X [N, c] device fp32 row-major, 16-byte aligned.  W1, W2: HOST arrays of E device pointers, W1[e] [h, c] and W2[e] [c, h]
 * (nn.Linear layout, no bias), each 16-byte aligned.  G [E, c] (16-byte aligned; null if and only if E == 1).  Wc [c, C].
 * logits [N, C] fp32, written.  Built for c = 512, h = 128, 1 <= E <= 8, 1 <= C <= 64; anything else is refused.
 * The bf16-term images of the weights are rebuilt in `workspace` on every call (moc_adapter_workspace bytes of device
 * memory, 16-byte aligned; 0 for shapes outside the limits): nothing is cached between calls.
 * Additive to ABI 20: the version number is unchanged. */
size_t moc_adapter_workspace(int64_t N, int c, int h, int E, int C);
int moc_adapter_logits(const float* X, int64_t N, int c, const float* const* W1, const float* const* W2, int h, int E,
                       const float* G /*nullable*/, const float* Wc, int C, float ratio, float* logits,
                       void* workspace, size_t workspace_bytes, moc_stream_t stream);

/* f3: the Nystrom attention layer of TransMIL (models/model_mil.py:105-122; moc_amd/nystrom.py),
 * forward only, for the no-grad passes.  Built for ONE shape -- heads = 8, dim_head = 64, landmarks = 256, a residual
 * convolution of at most 33 (odd) taps, batch 1 -- anything else is refused before a launch (moc_nystrom_workspace: 0).
 * qkv [n_pad, 1536] device fp32 as to_qkv leaves it, token-major: q of head h at columns 64 h .. 64 h + 63, k at 512 + 64 h,
 * v at 1024 + 64 h; n_pad a multiple of 256 (front-padding rows are ordinary rows: nothing is masked).
 *   moc_nystrom_landmark_values:  W[h] = softmax_over_tokens(q_l[h] k[h]^T) v[h]            W, q_l: [8, 256, 64]
 *       (q_l: the scaled segment means of q).  The token range is split in ranges of 512 whose (max, sum, accumulator)
 *       partials go through `ws` (moc_nystrom_workspace bytes) and are merged in index order: no atomics, same bits on
 *       every call.
 *   moc_nystrom_token_values:     out[i, 64 h ..] = softmax_256(scale q[i, h] k_l[h]^T) Y[h] + sum_t w[h, t] v[i + t - taps / 2, h]
 *       k_l, Y: [8, 256, 64]; conv_w [8, taps] (rows outside [0, n_pad) count as zero) or null for no residual (taps is
 *       then ignored); out [n_pad, 512] fp32, token-major, written.
 * All pointers 16-byte aligned.  Products are fp32 (v_mfma_f32_16x16x4_f32).  Additive to ABI 20: the version number is
 * unchanged. */
size_t moc_nystrom_workspace(int64_t n_pad, int heads, int dim_head, int landmarks);   /* 0: unsupported shape */
int moc_nystrom_landmark_values(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                const float* q_l /* [h, m, d], already scaled */, float* W /* [h, m, d] */,
                                void* ws, size_t ws_bytes, moc_stream_t stream);
int moc_nystrom_token_values(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                             const float* k_l, const float* Y, const float* conv_w /* [h, taps] or NULL */, int taps,
                             float scale, float* out /* [n_pad, h*d] */, moc_stream_t stream);

/* The backward of those two products, for training on them (moc_amd/nystrom.py: LandmarkValues, TokenValues).  The softmax
 * weights are recomputed tile by tile from the operands and one statistic per row; nothing of size n_pad x 256 is written.
 *   moc_nystrom_landmark_values_lse: moc_nystrom_landmark_values (the same two launches, the same bits in W) which also
 *       stores lse[h, m] = log sum_tokens exp(q_l[h, m] . k[h, token]), [8, 256].
 *   moc_nystrom_landmark_backward:   given dW [8, 256, 64]: dqkv's k and v columns (dk = dS^T q_l, dv = P^T dW with
 *       P = exp(S - lse), dS = P (dW v^T - dW . W)) and dq_l = dS k [8, 256, 64]; dqkv's q columns are written as zeros.
 *   moc_nystrom_token_backward:      the token product WITHOUT the residual convolution; given dout [n_pad, 512]: dqkv's q
 *       columns (scale dS k_l), dk_l = dS^T (scale q) and dY = P^T dout, both [8, 256, 64]; dqkv's k and v columns are
 *       written as zeros.
 * Each backward entry writes every element of its dqkv [n_pad, 1536].  `ws`: moc_nystrom_backward_workspace bytes, one size
 * for either backward entry (per-token statistics and the partial sums of each 512-token range, merged in index order: no
 * atomics, the same bits on every call), less than one [8, n_pad, 256] fp32 score matrix for every valid n_pad; the _lse
 * entry takes moc_nystrom_workspace bytes like the entry it extends.  MOC_EUNSUPPORTED for another shape; MOC_EINVAL for
 * a null or not 16-byte aligned pointer, a bad n_pad, a short workspace, a non-finite scale -- all before the first launch.
 * Additive to ABI 20: the version number is unchanged. */
size_t moc_nystrom_backward_workspace(int64_t n_pad, int heads, int dim_head, int landmarks);   /* 0: unsupported shape */
int moc_nystrom_landmark_values_lse(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                    const float* q_l, float* W, float* lse /* [h, m] */, void* ws, size_t ws_bytes,
                                    moc_stream_t stream);
int moc_nystrom_landmark_backward(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                  const float* q_l, const float* W, const float* lse, const float* dW,
                                  float* dqkv /* [n_pad, 3*h*d] */, float* dq_l /* [h, m, d] */,
                                  void* ws, size_t ws_bytes, moc_stream_t stream);
int moc_nystrom_token_backward(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                               const float* k_l, const float* Y, float scale, const float* dout /* [n_pad, h*d] */,
                               float* dqkv /* [n_pad, 3*h*d] */, float* dk_l, float* dY,
                               void* ws, size_t ws_bytes, moc_stream_t stream);

/* The backward of moc_nystrom_token_values' residual convolution, for training on kernel B WITH it (moc_amd/nystrom.py:
 * TokenValuesResidual).  With out[i, 64 h + d] += sum_t w[h, t] v[i + t - taps / 2, h, d] and dout [n_pad, 512]:
 *   dv[j, h, d] = sum_t w[h, t] dout[j - t + taps / 2, h, d]      written to dqkv's v columns (1024 + 64 h + d) ONLY: the q
 *       and k columns are not touched, so the entry runs in stream order after moc_nystrom_token_backward on the same dqkv
 *       and replaces that entry's zeros;
 *   dw[h, t]    = sum_i sum_d dout[i, h, d] v[i + t - taps / 2, h, d]      every element of dconv_w [8, taps] is written.
 * Rows outside [0, n_pad) count as zero and are not read.  dw is summed in fp32 over the 64 features of one (token, tap)
 * pair and in double above that; each 256-token block leaves 33 doubles per head in `ws`
 * (moc_nystrom_conv_backward_workspace bytes) and a merge launch adds the blocks in index order: no atomics, the same bits
 * on every call.  MOC_EUNSUPPORTED for another shape and for taps > 33; MOC_EINVAL for a null or not 16-byte aligned
 * pointer, a bad n_pad, taps < 1 or even, a short workspace -- all before the first launch.  Additive to ABI 20: the
 * version number is unchanged. */
size_t moc_nystrom_conv_backward_workspace(int64_t n_pad, int heads, int dim_head, int landmarks, int taps);  /* 0: unsupported */
int moc_nystrom_conv_backward(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                              const float* conv_w /* [h, taps] */, int taps, const float* dout /* [n_pad, h*d] */,
                              float* dqkv /* [n_pad, 3*h*d] */, float* dconv_w /* [h, taps] */,
                              void* ws, size_t ws_bytes, moc_stream_t stream);

/* The same layer's landmark pseudo-inverse (moc_amd/nystrom.py: moore_penrose_iter_pinv) as a chain of fp32 products on
 * the whole chip, for heads = 8 and landmarks = 256 only.  A = attn2 [8, 256, 256] device fp32, never written:
 *   c = max over all heads and rows of sum_j |A[h, i, j]|, r = likewise of the column sums;  Z0 = A^T / (c r)
 *   iters times:  XZ = A Z;  Z <- 0.25 Z (13 I - XZ (15 I - XZ (7 I - XZ)))
 * Z [8, 256, 256] receives the result (Z0 for iters = 0) and is written by the last product only.  Two init launches and
 * four products per iteration in stream order; no atomics, no grid-wide barrier: the same bits on every call.  The
 * intermediates live in `ws` (moc_nystrom_pinv_workspace bytes: five matrices and the partial maxima).  MOC_EUNSUPPORTED
 * for another shape; MOC_EINVAL for null or not 16-byte aligned pointers, A and Z (or ws) overlapping, a short workspace,
 * iters outside 0..64 -- all before the first launch.  Additive to ABI 20: the version number is unchanged. */
size_t moc_nystrom_pinv_workspace(int heads, int landmarks);          /* 0: unsupported shape */
int moc_nystrom_pinv(const float* A /* [h, m, m] */, int heads, int landmarks, int iters,
                     float* Z /* [h, m, m] */, void* ws, size_t ws_bytes, moc_stream_t stream);

/* moc_nystrom_pinv made to keep every iterate, for training (moc_amd/nystrom.py: LandmarkPinv): Zs[t] = Z_t for
 * t = 0 .. iters, and Zs[iters] is bit for bit what moc_nystrom_pinv returns.  The same launches, the same workspace size
 * (moc_nystrom_pinv_workspace), the same refusals, with Zs [(iters + 1), h, m, m] in Z's place. */
int moc_nystrom_pinv_iterates(const float* A /* [h, m, m] */, int heads, int landmarks, int iters,
                              float* Zs /* [iters + 1, h, m, m] */, void* ws, size_t ws_bytes, moc_stream_t stream);

/* The gradient through moc_nystrom_pinv_iterates: dA [h, m, m] from A, the iterates Zs and dZ = d(Zs[iters]).  For
 * t = iters - 1 .. 0, with XZ, P2, P3 recomputed from Z_t (only the iterates are saved):
 *   dP3 = -0.25 Z_t^T dZ;  dP2 = -(XZ^T dP3);  dXZ = dP3 (15 I - P2)^T + dP2 (7 I - XZ)^T - XZ^T dP2
 *   dA += dXZ Z_t^T;       dZ <- 0.25 dZ (13 I - P3)^T + A^T dXZ
 * then through Z0 = A^T / (c r):  dA += dZ^T / (c r);  dden = -sum(dZ o Z0) / (c r), one reduction in double in a fixed
 * order;  the rows whose sum of |A| IS c share dden r evenly, each of their elements + share x sign(A) (torch's rule for a
 * full max(); sign(0) = 0), and the columns whose sum IS r share dden c likewise -- the sums are the forward's own code.
 * Products of one to three terms with either operand transposed on the way into LDS, independent products side by side in
 * one launch: 3 + 4 iters product launches and four for the init, 31 at six iterations, in stream order; no atomics, no
 * grid-wide barrier: the same bits on every call.  Every element of dA is written; no input is.  `ws` holds
 * moc_nystrom_pinv_backward_workspace bytes (eleven matrices, the sums, the partials).  MOC_EUNSUPPORTED for another
 * shape; MOC_EINVAL for null or not 16-byte aligned pointers, any two of A, Zs, dZ, dA and ws overlapping, a short
 * workspace, iters outside 0..64 -- all before the first launch.  Additive to ABI 20: the version number is unchanged. */
size_t moc_nystrom_pinv_backward_workspace(int heads, int landmarks);  /* 0: unsupported shape */
int moc_nystrom_pinv_backward(const float* A /* [h, m, m] */, int heads, int landmarks, int iters,
                              const float* Zs /* [iters + 1, h, m, m] */, const float* dZ /* [h, m, m] */,
                              float* dA /* [h, m, m] */, void* ws, size_t ws_bytes, moc_stream_t stream);

/* Rows of the same layer's attention matrix attn1 pinv attn3, for attention maps (moc_amd/nystrom.py:
 * NystromAttention.forward_rows).  With lse what moc_nystrom_landmark_values_lse returns for the same qkv and q_l, and
 * coef[h, r, :] = softmax_256(scale q[i_r, h] k_l[h]^T) pinv[h] the caller's 256-vector per head and wanted row i_r:
 *   out[h, r, j] = sum_m coef[h, r, m] exp(q_l[h, m] . k[j, h] - lse[h, m])          r < R, j < n_pad
 * One launch of one workgroup per head and 256 tokens; attn3, the [8, 256, n_pad] score matrix, is not formed; no running
 * maximum (s - lse <= 0 up to rounding), no workspace, no atomics: the same bits on every call.  Every output is four fp32
 * chains (landmark tile lt in chain lt & 3, in index order) added pairwise.  Every element of out [8, R, n_pad] is written; no input is.
 * MOC_EUNSUPPORTED for another head, landmark or dim_head shape and for n_pad above 2^22; MOC_EINVAL for n_pad not a positive
 * multiple of 256, R outside 1..16, a null or not 16-byte aligned pointer, out overlapping qkv, q_l, lse or coef -- all
 * before the launch.  Additive to ABI 20: the version number is unchanged. */
int moc_nystrom_attention_rows(const float* qkv /* [n_pad, 1536] */, int64_t n_pad, int heads, int dim_head, int landmarks,
                               const float* q_l /* [8, 256, 64], scaled */, const float* lse /* [8, 256] */,
                               const float* coef /* [8, R, 256] */, int R, float* out /* [8, R, n_pad] */, moc_stream_t stream);

/* TransMIL's PPEG (moc_amd/model_mil.py: PPEG): the depth-wise 7 x 7, 5 x 5 and 3 x 3 convolutions over the H x W token
 * square, the identity and the three biases in one launch, and their gradients in two.  x, out, dout, dx are
 * [1 + H W, dim] device fp32, row 0 the class token, row 1 + y W + x_ position (y, x_); w7 [dim, 1, 7, 7], w5 [dim, 1, 5, 5],
 * w3 [dim, 1, 3, 3] and the biases [dim] as nn.Conv2d stores them.  With zero padding outside the square, p a position:
 *   out[0]        = x[0]
 *   out[1 + p, c] = x[1 + p, c] + ((b7[c] + b5[c]) + b3[c]) + sum_{dy, dx in -3..3} w[c, dy, dx] x[1 + p + (dy, dx), c]
 *                   w = (w7 + pad(w5)) + pad(w3): one 7 x 7 table per channel, the 5 x 5 and the 3 x 3 in its centre
 *   dx[0]         = dout[0]
 *   dx[1 + p, c]  = dout[1 + p, c] + sum_{dy, dx} w[c, dy, dx] dout[1 + p - (dy, dx), c]
 *   G[c, dy, dx]  = sum_p dout[1 + p, c] x[1 + p + (dy, dx), c]
 *   dw7 = G;  dw5 = G's central 5 x 5;  dw3 = G's central 3 x 3;  db7 = db5 = db3 = sum_p dout[1 + p, c]
 * Positions outside the square count as zero and are not read.  Every element of out, of dx and of the six gradient
 * tensors is written; no input is.  An output is one fp32 chain of 49 products; G and the bias sum are added in fp32 over
 * at most 64 products and in double above that: each block of at least 128 positions leaves 50 doubles per channel in `ws`
 * (moc_ppeg_backward_workspace bytes: at most 2 MiB while H W < 1,024, below one [H W, 512] fp32 tensor from there on) and
 * a merge launch adds the blocks in index order and rounds to fp32 once: no atomics, the same bits on every call.  Built
 * for dim = 512, H, W >= 1, H W <= 2^22.  MOC_EUNSUPPORTED for another dim; MOC_EINVAL for a null or not 16-byte aligned
 * pointer, H or W below 1 or a product above the limit, a short workspace, out overlapping x, dx overlapping dout or x
 * (the halo is read after neighbours are written: in place cannot work) -- all before the first launch.  Additive to ABI
 * 20: the version number is unchanged. */
int moc_ppeg_forward(const float* x /* [1 + H W, dim] */, int H, int W, int dim, const float* w7, const float* b7,
                     const float* w5, const float* b5, const float* w3, const float* b3, float* out /* [1 + H W, dim] */,
                     moc_stream_t stream);
size_t moc_ppeg_backward_workspace(int H, int W, int dim);            /* 0: unsupported shape */
int moc_ppeg_backward(const float* x /* [1 + H W, dim] */, int H, int W, int dim, const float* w7, const float* w5,
                      const float* w3, const float* dout /* [1 + H W, dim] */, float* dx /* [1 + H W, dim] */, float* dw7,
                      float* db7, float* dw5, float* db5, float* dw3, float* db3, void* ws, size_t ws_bytes,
                      moc_stream_t stream);

/* a10-a15 fused: `n` consecutive meta-steps (one slide each, slides slide0..slide0+n-1 in
 * order, one Adam step per slide: main_moc.py:380-410), parameters and Adam moments
 * updated in place.  Per-slide loss/pooled land in ws->loss / ws->pooled. */
int moc_train_steps(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                    const int64_t* labels, int slide0, int n, uint32_t use_bits,
                    moc_stream_t stream);

/* How often moc_train_steps knew a step's selected-row count on the host (moc_batch_t.n_sel_host or a valid word of
 * n_sel_mail) before it launched the step: process-wide counters of the steps it has issued and of those among them with
 * a host count.  Either pointer may be NULL; reset != 0 zeroes both after reading.  Tests and measurements read the
 * share here, without a profiler.  Additive to ABI 20 (as the two mailbox fields at the end of moc_batch_t are): the
 * version number is unchanged. */
int moc_n_sel_stats(int64_t* known, int64_t* steps, int reset);

/* The same pass as ONE graph launch (main_moc.py:380-410: the whole `for data in train_loader` body, n slides).
 * moc_train_steps issues 2 n + 1 kernel launches; at the start of a run -- or of a short timed region -- the stream is
 * empty and the chain of 20-us meta-steps cannot run ahead of the host.  A `moc_step_graph_t` keeps each distinct pass
 * (work arrays, meta-learner tensors, slide range) as an instantiated hipGraph and replays it with one call.  It is the
 * second explicit handle of this ABI (after moc_p2p_t): it owns host-side state only -- the graphs, one pinned staging
 * buffer, an event; the device memory it uses is the caller's `device_ws` (moc_step_graph_workspace_bytes(max_steps):
 * a step counter + the Adam coefficients of the next max_steps steps, which the captured kernels read by position
 * because kernel arguments are frozen at capture while the bias corrections change with every step).
 *   - results are bit-identical to moc_train_steps (same kernels, same coefficient floats);
 *   - all calls on one handle must be ordered on one stream (the counter lives in stream order);
 *   - M->step is read on every call: if it is not where the handle left it (another optimizer stepped, a checkpoint
 *     was loaded), the device counter is put right first; new hyper-parameters or an exhausted table rebuild the table;
 *   - B->n_sel_host, B->n_sel_mail and B->n_sel_ticket are ignored: a captured pass reads the device n_sel, whichever
 *     pass it was captured in (the stream-launch fall-back below does use them);
 *   - shapes outside the one-launch steps, n > max_steps, or a runtime that refuses capture / instantiation fall back
 *     to moc_train_steps (moc_step_graph_stats tells which path ran).
 * The caller advances M->step by n afterwards, as with moc_train_steps. */
typedef struct moc_step_graph moc_step_graph_t;
size_t moc_step_graph_workspace_bytes(int max_steps);
int moc_step_graph_create(void* device_ws, size_t ws_bytes, moc_step_graph_t** out);
int moc_step_graph_destroy(moc_step_graph_t* G);
int moc_step_graph_stats(const moc_step_graph_t* G, int* captures, int* replays, int* eager_calls);
int moc_train_steps_graph(moc_step_graph_t* G, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                          const int64_t* labels, int slide0, int n, uint32_t use_bits, moc_stream_t stream);

/* ---- compute units kept free of the score pass (round 3) -----------------------------------------------------------
 * Phase A of the NEXT pass (main_moc.py:322-375 for every slide: no trainable parameter) is issued a pass ahead on a
 * side stream while the sequential meta-steps of this pass (main_moc.py:380-410) run.  The score pass fills every CU
 * with persistent workgroups, and a 16-wave meta-step workgroup fits on no CU that holds one of them: the meta-steps
 * stalled for the length of the score pass.  (Confining the side stream's queue with a CU mask,
 * hipExtStreamCreateWithCUMask, was measured: the masked queue is not scheduled beside the unmasked one at all -- the
 * rate halves; profiles/NOTES.md.)  Instead the score pass itself stays off a set of compute units:
 *   moc_batch_t.tile_ticket  (device int32[MOC_TICKET_WORDS], nullable): the score pass hands out its 16-row tiles
 *       through MOC_TICKET_QUEUES counters (eight per XCD, 256 bytes apart, two tiles per ticket; a wave whose own has
 *       run out takes from any other; eight more words rank the workgroups of each XCD) instead of a static stride per
 *       wave, so any number of its workgroups can do all the work (moc_scores zeroes them in stream order before each
 *       launch);
 *   moc_batch_t.cu_reserved  (device uint32[128], nullable; needs tile_ticket): bit (xcc * 256 + HW_ID[15:8]) set = a
 *       workgroup of the score pass that finds itself on that compute unit ends at once (the first eight workgroups of
 *       a launch never do: progress does not depend on the table being right).
 * moc_cu_census finds out which (xcc, HW_ID[15:8]) slots the device has: it launches `n_wg` one-wave workgroups that
 * each hold their CU for ~`hold_us` microseconds and counts them in hist[xcc * 256 + HW_ID[15:8]] (device int32
 * [16 * 256], zeroed by the caller).  The host picks the reserved slots from it (moc_amd/engine.py: reserved_cus). */
int moc_cu_census(int32_t* hist, int n_wg, int hold_us, moc_stream_t stream);

/* ---- generic pooling / ranking (a12, a17 and the index_* helpers) ----------
 * For each segment s (rows seg_off[s] .. seg_off[s+1]) and class c: rank rows by
 * keys[c*key_stride + row] (largest first, or smallest first when `smallest`),
 * take k = min(K, len) and write mean(vals[c*val_stride + row]) over them to
 * pooled[s*C + c] (utils/patch_selection_classifier.py:18-32, :35-80, :127-171).
 * idx_out (nullable, int32 [n_seg, C, K]): chosen rows relative to the segment,
 * ordered by key (ties: lower row first); cnt_out (nullable) [n_seg, C].
 * K <= 4096. */
int moc_topk_mean(const float* keys, int64_t key_stride, const float* vals, int64_t val_stride,
                  const int64_t* seg_off, const int32_t* seg_len /*nullable*/, int n_seg, int C, int K,
                  int smallest, float* pooled, int32_t* idx_out, int32_t* cnt_out,
                  moc_stream_t stream);

/* ---- pooling at several K from one ranking (sensitivity sweeps) ----------
 * For each segment s and class c: rank as moc_topk_mean does (largest first, or smallest first when `smallest`; ties:
 * lower row first) ONCE to Kmax = max(Ks), and for every i write the mean of the first min(Ks[i], len) values, summed
 * in rank order, to pooled[(i * n_seg + s) * C + c] -- bit for bit moc_topk_mean at K = Ks[i].
 * Ks: HOST array, 1 <= n_K <= 8, every K in [1, 64], any order, repeats allowed.
 * idx_out (nullable) int32 [n_seg, C, Kmax], cnt_out (nullable) [n_seg, C] = min(Kmax, len): as moc_topk_mean at Kmax
 * (an empty segment's idx_out row is all -1).  An empty segment pools to NaN for every K.
 * Additive to ABI 20: the version number is unchanged. */
int moc_topk_mean_multi(const float* keys, int64_t key_stride, const float* vals, int64_t val_stride,
                        const int64_t* seg_off, const int32_t* seg_len /*nullable*/, int n_seg, int C,
                        const int32_t* Ks, int n_K, int smallest, float* pooled, int32_t* idx_out, int32_t* cnt_out,
                        moc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOC_HIP_H */
