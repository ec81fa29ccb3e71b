/*
 * eeg_dcrnn.h — C ABI of libeeg_dcrnn_hip.so: MI355X (gfx950) kernels for the DCRNN hot path of
 * tsy935/eeg-gnn-ssl (model/cell.py DiffusionGraphConv + DCGRUCell, and the encoder sequence
 * loop of model/model.py).  Plain pointers and sizes only; every pointer is a DEVICE pointer to
 * contiguous fp32 (int64 for lengths) unless stated; `stream` is a hipStream_t passed as void*.
 * All functions enqueue work on `stream` and return without synchronising; they never allocate.
 * Return value: 0 on success, non-zero on error (see eeg_dcrnn_last_error()).
 * Empty operands (zero clips, zero steps, zero widths) are an error of every compute entry, raised before anything is launched --
 * the reference raises on them too (model.py:253-255: its reshape(..., -1) of a tensor without elements); the host-only size /
 * capability queries (size_t eeg_dcrnn_*_floats, eeg_dcrnn_supported, *_ok, *_is_persistent) never fail and return 0 for such dims.
 *
 * The reference has no FFI of its own (pure Python); each entry point below states
 * the reference code it replaces.  The ctypes binding that a maintainer of the reference would
 * add is shown in INTEGRATION.md and lives in eeg_gnn_ssl_amd/_lib.py.
 *
 * Layouts.  N = nodes (<= 32), H = rnn_units (16 | 32 | 64), F/Fin = per-node input features of a
 * layer (multiple of 4), M = number of hop matrices incl. identity = n_supports*K + 1 (<= 8),
 * S = T*B "samples" in time-major order (s = t*B + b).
 *   supports : n_supports pointers, each (G, N, N) with G = B (per-clip graphs) or 1 (shared)
 *   P        : (G, M-1, N, N) hop-polynomial matrices P_1..P_{M-1} (P_0 = I is implicit)
 *   X        : (T, B, N, Fin)            planes : (M-1, S, N, Fin)  = P_m X_s, m = 1..M-1
 *   Hext     : (T+1, B, N, H)  slot 0 = initial state h0, slot t+1 = h_t  (so the layer output
 *              sequence is Hext + B*N*H and the "previous state" sequence is Hext itself)
 *   Rs,Us,Cs,RHs : (T, B, N, H) saved reset gate, update gate, candidate, r*h_prev
 *   Wg (((Fin+H)*M), 2H), bg (2H), Wc (((Fin+H)*M), H), bc (H): reference parameter layout,
 *              row = f*M + m  (cell.py:40-46, 98-116)
 */
#ifndef EEG_DCRNN_H
#define EEG_DCRNN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eeg_layer_dims {
    int32_t T, B, N, H, Fin, M;
    int32_t act;        /* 0 = tanh, 1 = relu  (cell.py:146 `nonlinearity`) */
    int32_t p_batched;  /* 1: P holds one graph per clip (B graphs); 0: one shared graph */
    int32_t x_planes_ready;  /* 1: `planes` already holds P_m X (the previous layer's Hplanes, slots 1..T) */
    int32_t x_batch_major;   /* 1: X is the BATCH-major (B,T,N,Fin) model input and is consumed as it is; `planes` then
                                holds P_m X in the same (b,t) order and the hoisted GEMMs address both through a row
                                map: no time-major copy is written (only where eeg_dcrnn_batch_major_ok() returns 2;
                                pass the same X and planes to layer_bwd) */
    int64_t x_plane_stride;  /* floats between two hop planes of `planes`; 0 = T*B*N*Fin (contiguous) */
    const uint16_t* pack3;   /* OPT-IN (NULL = off, the default and the contract's arithmetic): the cell's three-term bf16 weight packs
                                of eeg_dcrnn_pack_cell_bf16x3.  When set, the two hoisted NN GEMMs of the layer -- the x-part
                                pre-activations (layer_fwd) and the input gradient (layer_bwd) -- run as a three-term bf16 split
                                (6 of the 9 partial products) on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: fp32 operands and
                                results, error against an fp64 sum at the level of the fp32 matrix pipe's own (~2e-6 on values
                                of a few units), 1.3-1.4 x its speed.  Everything else of the layer is unchanged. */
    const float* spectral;   /* NULL = off.  Else: the eeg_dcrnn_spectral_basis block of the ONE symmetric support all clips share
                                (p_batched = 0; the scaled Laplacian of the distance graph, filter_type "laplacian") and `spack` the
                                cell's per-frequency weight packs (eeg_dcrnn_pack_cell_spectral).  The hoisted x-part of the layer
                                then runs in the eigenbasis of the support: all hop matrices are Chebyshev polynomials of one
                                symmetric S = U diag(lam) U^T (cell.py:83-93), so sum_m P_m X W_m = U [ (U^T X)_i Wt_i ]_i with
                                Wt_i = sum_m T_m(lam_i) W_m -- the GEMMs contract over Fin instead of M*Fin; the node mixes with U / U^T
                                run inside the recurrent kernels and the input-gradient GEMM (one pass is left: U^T of the layer-0
                                input); backward likewise.  Exact up to re-association (~1e-6); the recurrence is unchanged.
                                Only where eeg_dcrnn_spectral_ok() says so.  `planes` of layer_fwd / layer_bwd is then the
                                node-major transformed input Xh (N, eeg_dcrnn_spectral_rows(T*B), Fin) (written by layer_fwd, read
                                by layer_bwd) and x_planes_ready must be 0. */
    const float* spack;
} eeg_layer_dims;

typedef struct eeg_decoder_dims {
    int32_t T, B, N, H;  /* T = output horizon (decoder steps) */
    int32_t Dout;        /* output_dim = input_dim of the first decoding cell (model.py:131-143) */
    int32_t M, L;        /* hop matrices; num_rnn_layers (layers >= 1 share ONE cell, model.py:126-143) */
    int32_t act, p_batched;
    float dropout_p;     /* nn.Dropout in front of the projection (model.py:191), p when the module is training, else 0 */
    int32_t teacher_on_device;  /* 1: `teacher` of decoder_fwd / _bwd is a DEVICE int32[T] array (e.g. written by
                                   eeg_dcrnn_teacher_flags earlier on the stream) that the persistent kernels read when they
                                   start -- a captured HIP graph then replays with fresh curriculum-learning flags; 0: HOST array */
} eeg_decoder_dims;

/* Human-readable text of the last error raised on the calling thread. */
const char* eeg_dcrnn_last_error(void);
/* ABI version (bumped on any signature change). */
int eeg_dcrnn_abi_version(void);
/* 1 if the library was built for the GPU (always, for the product build), 0 for the test emulator. */
int eeg_dcrnn_is_device_build(void);
/* 1 if kernels are instantiated for this (N, H, Fin, M); else 0 and last_error says why. */
int eeg_dcrnn_supported(int N, int H, int Fin, int M);

/* Clears `bytes` bytes at p on the stream (one small kernel node in a captured graph): `optimizer.zero_grad()` on the flat gradient
 * bucket (train.py:262) and the never-read slot 0 of an upper layer's input gradient, without a framework fill kernel. */
int eeg_dcrnn_zero(void* p, size_t bytes, void* stream);

/* Hop polynomials from the supports (replaces the per-step `torch.matmul(support, x)` chain of
 * cell.py:83-93 incl. the carried-x0 quirk): P_out (G, n_supports*K, N, N). */
int eeg_dcrnn_hop_polys(const float* const* supports, int n_supports, int n_graphs, int N, int K,
                        float* P_out, void* stream);

/* Input featurisation (replaces the DataLoader-side CPU code: data_utils.py:13-35 `computeFFT` applied to
 * every 1-second step as dataloader_detection.py:57-71 does; :233-256 augmentation; utils.py:393-428
 * StandardScaler.transform).  raw (B,N,T*W) resampled signals; W = samples per step (200).
 *   feat_raw (B,T,N,W/2), nullable : log|FFT| of the W/2 positive frequencies (amp == 0 -> 1e-8), the
 *                                    un-augmented clip the correlation graph is built from;
 *   feat_std (B,T,N,W/2), nullable : ((log|FFT| of channel perm[b][n]) + log_scale[b] - mean) / std,
 *                                    the model input.  perm (B,N) int32 / log_scale (B) may be NULL
 *                                    (no reflection / no amplitude jitter).  The transform runs in fp64. */
int eeg_dcrnn_fft_features(const float* raw, int B, int N, int T, int W, const int32_t* perm,
                           const float* log_scale, float mean, float std_, float* feat_raw,
                           float* feat_std, void* stream);

/* Variable-length clips (the classification loader: dataloader_classification.py:25-85 cuts a clip of curr_len <= max_seq_len
 * steps, :321-343 augments and standardises the short clip and THEN pads it to max_seq_len with padding_val; :356-361 builds the
 * correlation graph of the unpadded clip).  eeg_dcrnn_fft_features with lengths (B) int64 ON THE DEVICE (read by the kernel: the
 * launch does not depend on them, a captured launch replays with new lengths): clip b has len_b = clamp(lengths[b], 1, T) valid
 * windows.  A window (b, n, t >= len_b) is not transformed: its feat_std row is pad_val, its feat_raw row 0 (a zero row adds nothing
 * to a Gram).  Valid windows are bit-identical to eeg_dcrnn_fft_features; W = 200 skips the padding six windows at a time. */
int eeg_dcrnn_fft_features_len(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* log_scale, float mean,
                               float std_, const int64_t* lengths, float pad_val, float* feat_raw, float* feat_std, void* stream);

/* The data side of the SSL sample, which is a PAIR (dataloader_ssl.py:317-341): 60 s of input and the first seconds of the
 * following clip as target; ONE coin and ONE scale factor per sample (`_random_reflect(…, reflect)` / `_random_scale(…,
 * scale_factor)`, dataloader_ssl.py:159-182) applied to both halves, then the StandardScaler on both.  raw_x (B,N,Tx*W),
 * raw_y (B,N,Ty*W); perm (B,N) int32 / log_scale (B) as for eeg_dcrnn_fft_features, nullable (no augmentation).
 *   feat_raw_x (B,Tx,N,W/2), nullable : log|FFT| of the un-reflected, un-scaled INPUT clip, the operand of the correlation
 *                                       graph (dataloader_ssl.py:349; the target plays no part in the graph);
 *   x_std (B,Tx,N,W/2), y_std (B,Ty,N,W/2) : ((log|FFT| of channel perm[b][n]) + log_scale[b] - mean) / std of each half.
 * W = 200: both halves in ONE launch; every output is bit-identical to eeg_dcrnn_fft_features on that half (the same transform,
 * re-scheduled).  Any other W: the general kernel of eeg_dcrnn_fft_features, once per half. */
int eeg_dcrnn_fft_features_pair(const float* raw_x, const float* raw_y, int B, int N, int Tx, int Ty, int W, const int32_t* perm,
                                const float* log_scale, float mean, float std_, float* feat_raw_x, float* x_std, float* y_std,
                                void* stream);

/* The same augmentation on an SSL pair of already STANDARDISED features (dataloader_ssl.py:159-182,317-341 followed by
 * utils.py:393-428: reflecting commutes with the scaler, and adding log(scale) before it = adding log(scale) / std behind it):
 *   x_out[b,t,n,:] = x[b,t,perm[b][n],:] + shift[b],   y_out likewise,   shift[b] = log_scale[b] / std.
 * x, x_out (B,Tx,N,D); y, y_out (B,Ty,N,D); D % 4 == 0, 16-byte aligned, outputs distinct from inputs.  One launch, one read and
 * one write of every value (HBM-bound: algorithmic bytes 8*B*(Tx+Ty)*N*D); a perm entry outside 0..N-1 selects the node itself. */
int eeg_dcrnn_augment_features(const float* x, const float* y, int B, int Tx, int Ty, int N, int D, const int32_t* perm,
                               const float* shift, float* x_out, float* y_out, void* stream);

/* Time-domain inputs (the reference without --use_fft), replacing the DataLoader-side CPU code: dataloader_detection.py:25-85
 * `computeSliceMatrix(is_fft=False)` (clip[t,n,:] = raw[n, t*W:(t+1)*W]), :233-245 `_random_reflect`, :247-256 `_random_scale`
 * (`EEG_seq *= scale_factor`), utils.py:393-428 StandardScaler.transform.  raw (B,N,T*W) resampled signals, W % 4 == 0;
 *   x_std (B,T,N,W) : (raw[b, perm[b][n], t*W ..] * scale[b] - mean) / std in fp32, the model input.
 * perm (B,N) int32 / scale (B) may be NULL (no reflection / factor 1); a perm entry outside 0..N-1 selects the node itself.
 * No un-augmented copy is written: the correlation graph of a time-domain clip is that of the raw rows (eeg_dcrnn_corr_graph_rows).
 * One read and one write of every value (HBM-bound: algorithmic bytes 8*B*N*T*W); tensors 16-byte aligned. */
int eeg_dcrnn_window_features(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* scale, float mean,
                              float std_, float* x_std, void* stream);

/* eeg_dcrnn_window_features for variable-length clips (dataloader_classification.py:25-85,321-343: the short clip is scaled and
 * standardised, then padded): lengths (B) int64 on the device, len_b = clamp(lengths[b], 1, T); the steps t >= len_b of clip b are
 * not loaded and x_std holds pad_val there; every other value is bit-identical to eeg_dcrnn_window_features. */
int eeg_dcrnn_window_features_len(const float* raw, int B, int N, int T, int W, const int32_t* perm, const float* scale, float mean,
                                  float std_, const int64_t* lengths, float pad_val, float* x_std, void* stream);

/* The same for the SSL pair (dataloader_ssl.py:159-182,317-341: one coin and one scale factor per sample on input AND target, the
 * scaler on both): raw_x (B,N,Tx*W), raw_y (B,N,Ty*W) -> x_std (B,Tx,N,W), y_std (B,Ty,N,W) in ONE launch; every output is
 * bit-identical to eeg_dcrnn_window_features on that half. */
int eeg_dcrnn_window_features_pair(const float* raw_x, const float* raw_y, int B, int N, int Tx, int Ty, int W, const int32_t* perm,
                                   const float* scale, float mean, float std_, float* x_std, float* y_std, void* stream);

/* The time-domain augmentation on already STANDARDISED windows (dataloader_detection.py:233-256 / dataloader_ssl.py:159-182 in
 * front of utils.py:393-428: (v*s - mean)/std = ((v - mean)/std)*s + (s - 1)*mean/std):
 *   x_out[b,t,n,:] = x[b,t,perm[b][n],:] * a[b] + c[b],   a[b] = s_b,   c[b] = (s_b - 1) * mean / std   (product rounded first),
 * and y_out likewise.  x, x_out (B,Tx,N,D); y, y_out (B,Ty,N,D), or y = y_out = NULL with Ty = 0 (the supervised tasks);
 * D % 4 == 0, 16-byte aligned, outputs distinct from inputs.  One launch, algorithmic bytes 8*B*(Tx+Ty)*N*D. */
int eeg_dcrnn_augment_windows(const float* x, const float* y, int B, int Tx, int Ty, int N, int D, const int32_t* perm, const float* a,
                              const float* c, float* x_out, float* y_out, void* stream);

/* Per-clip correlation graph and its dual random-walk supports, from the clips themselves
 * (replaces the DataLoader-side CPU code: dataloader_detection.py:258-307 `_get_indiv_graphs`
 * = |normalised lag-0 cross-correlation| of every electrode pair of the (N, T*D) clip, diag 1;
 * data_utils.py:174-200 keep_topk(top_k, directed=True); dataloader_detection.py:346-349 +
 * utils.py:220-230: S1 = (D^-1 A)^T, S2 = (D_in^-1 A^T)^T).  X (B,T,N,D) batch-major clips;
 * adj (B,N,N) may be NULL; S1, S2 (B,N,N).  HBM-bound: algorithmic bytes 4*B*T*N*D. */
size_t eeg_dcrnn_corr_graph_ws_floats(int B, int T);
int eeg_dcrnn_corr_graph(const float* X, int B, int T, int N, int D, int top_k, float* adj, float* S1,
                         float* S2, float* ws, void* stream);

/* The graph of the UNPADDED clip (dataloader_classification.py:356-361 on the clip of :25-85): only the steps t < len_b =
 * clamp(lengths[b], 1, T) of clip b enter the Gram, whatever the padded steps hold; lengths (B) int64 on the device.
 * ws: eeg_dcrnn_corr_graph_ws_floats(B, T) floats, as for eeg_dcrnn_corr_graph. */
int eeg_dcrnn_corr_graph_len(const float* X, int B, int T, int N, int D, int top_k, const int64_t* lengths, float* adj, float* S1,
                             float* S2, float* ws, void* stream);

/* The same graph from WIDE channel rows (time-domain clips: dataloader_detection.py:258-307 on a clip of :25-85, whose
 * `eeg_clip.reshape((num_sensors, -1))` is the raw (N, T*200) rows again).  The row of node n of clip b is P pieces of Q floats,
 * piece p at X[b*clip + p*piece_stride + n*Q ..]: raw rows (B,N,L) are P = 1, Q = L (piece_stride ignored); a window tensor
 * (B,T,N,D) is P = T, Q = D, piece_stride = N*D.  Q % 4 == 0 (no upper limit), N <= 32, a clip < 2 GB.  Normalisation, top-k and
 * supports are the code of eeg_dcrnn_corr_graph; fixed-order sums (bit-reproducible).  HBM-bound: algorithmic bytes 4*B*N*P*Q.
 * ws: eeg_dcrnn_corr_graph_rows_ws_floats(B, P, Q) floats. */
size_t eeg_dcrnn_corr_graph_rows_ws_floats(int B, int P, int Q);
int eeg_dcrnn_corr_graph_rows(const float* X, int B, int N, int P, int Q, long long piece_stride, int top_k, float* adj, float* S1,
                              float* S2, float* ws, void* stream);

/* eeg_dcrnn_corr_graph_rows of the UNPADDED clip (dataloader_classification.py:356-361 on a time-domain clip of :25-85): `steps` =
 * the steps of a full clip, len_b = clamp(lengths[b], 1, steps), lengths (B) int64 on the device.  Raw rows (P = 1): Q = steps * w
 * with w % 4 == 0, and the first len_b * w floats of every row enter the Gram (the row stride stays Q); window tensors: steps = P,
 * and the first len_b pieces do.  ws: eeg_dcrnn_corr_graph_rows_ws_floats(B, P, Q) floats. */
int eeg_dcrnn_corr_graph_rows_len(const float* X, int B, int N, int P, int Q, long long piece_stride, int top_k, const int64_t* lengths,
                                  int steps, float* adj, float* S1, float* S2, float* ws, void* stream);

/* Number of floats of the packed weight block of one DCGRU cell. */
size_t eeg_dcrnn_pack_floats(int Fin, int H, int M);
/* Reference-layout parameters of one cell (cell.py:40-46,160-175) -> MFMA-fragment-ordered block. */
int eeg_dcrnn_pack_cell(const float* Wg, const float* bg, const float* Wc, const float* bc,
                        int Fin, int H, int M, float* pack, void* stream);

/* Three-term bf16 packs (hi / mid / lo, round to nearest even) of the x-part weights of one cell for eeg_layer_dims.pack3:
 * eeg_dcrnn_pack3_halves() 16-bit elements; available for rnn_units = 64 (else 0 / an error). */
size_t eeg_dcrnn_pack3_halves(int Fin, int H, int M);
int eeg_dcrnn_pack_cell_bf16x3(const float* Wg, const float* Wc, int Fin, int H, int M, uint16_t* pack3, void* stream);

/* Spectral form of the hoisted x-part for a shared symmetric support (eeg_layer_dims.spectral).
 *   eeg_dcrnn_spectral_basis: support (N,N) -> basis block of eeg_dcrnn_spectral_basis_floats(N) floats:
 *       U (N*N; column i = eigenvector i) | T_m(lam_i) as [8][32] | info[32]: info[0] = max |S - U diag(lam) U^T| (it contains the
 *       asymmetry of S: a caller reads it ONCE per support and keeps the general path when it is not at rounding level),
 *       info[1] = largest off-diagonal left by the Jacobi sweeps, info[2] = max |S|.  One workgroup, fp64, ~50 us: once per
 *       support, not per step.
 *   eeg_dcrnn_pack_cell_spectral: the cell's x-part weights (reference layout) -> per-frequency packs Wt_i, Wt_i^T.
 *   eeg_dcrnn_spectral_ok: 1 if layer_fwd / layer_bwd (with or without an input gradient) take d->spectral for this shape
 *       (64 units, Fin % 4 == 0; need_dx: Fin == 64), else 0.  eeg_dcrnn_spectral_rows(S) = rows per frequency (S rounded up to 16). */
size_t eeg_dcrnn_spectral_basis_floats(int N);
int eeg_dcrnn_spectral_basis(const float* support, int N, float* basis, void* stream);
size_t eeg_dcrnn_spectral_pack_floats(int Fin, int H, int M, int N);
int eeg_dcrnn_pack_cell_spectral(const float* Wg, const float* Wc, const float* basis, int Fin, int H, int M, int N,
                                 float* spack, void* stream);
/* The packs of ALL cells of an encoder in ONE launch (their weights change with every optimisation step, cell.py:40-46):
 * cell c: eeg_dcrnn_pack_cell(Wg[c], bg[c], Wc[c], bc[c], Fin[c], H, M, packs[c]) and, when basis / spacks are given,
 * eeg_dcrnn_pack_cell_spectral(Wg[c], Wc[c], basis, Fin[c], H, M, N, spacks[c]).  The pointer TABLES are host arrays of
 * device pointers (n_cells <= 4); basis and spacks are NULL together. */
int eeg_dcrnn_pack_cells(int n_cells, const float* const* Wg, const float* const* bg, const float* const* Wc,
                         const float* const* bc, const int32_t* Fin, int H, int M, float* const* packs, const float* basis,
                         int N, float* const* spacks, void* stream);
int eeg_dcrnn_spectral_ok(const eeg_layer_dims* d, int need_dx);
size_t eeg_dcrnn_spectral_rows(size_t S);

/* The HBM-bound diffusion step over all samples: planes[m-1][s] = P_m X_s  (cell.py:83-93 applied
 * to the input features of every time step at once).  Algorithmic bytes: 4*S*N*F*M. */
int eeg_dcrnn_diffuse_fwd(const float* X, const float* P, int p_batched, int S, int B, int N, int F,
                          int M, float* planes, void* stream);
/* Adjoint: dX[s] = Z_0[s] + sum_{m>=1} P_m^T Z_m[s] for Z (S, N, M*F). */
int eeg_dcrnn_diffuse_adj(const float* Z, const float* P, int p_batched, int S, int B, int N, int F,
                          int M, float* dX, void* stream);

/* DiffusionGraphConv.forward (cell.py:66-118) on its own: X (B,N,F) = [inputs | state] per node,
 * W ((F*M), O) and bias (O) in reference layout, out (B,N,O). */
size_t eeg_dcrnn_dconv_fwd_ws_floats(int B, int N, int F, int M, int O);
int eeg_dcrnn_dconv_fwd(const float* X, const float* P, int p_batched, int B, int N, int F, int M,
                        const float* W, const float* bias, int O, float* out, float* ws, void* stream);

/* Backward of the same convolution (autograd's replay of cell.py:66-118): dOut (B,N,O) ->
 * dX (B,N,F), dW ((F*M), O) and dbias (O) in reference layout (each output may be NULL).  O <= 192. */
size_t eeg_dcrnn_dconv_bwd_ws_floats(int B, int N, int F, int M, int O);
int eeg_dcrnn_dconv_bwd(const float* X, const float* P, int p_batched, int B, int N, int F, int M,
                        const float* W, int O, const float* dOut, float* dX, float* dW, float* dbias,
                        float* ws, void* stream);

/* One DCGRU layer over a whole sequence = the `for t` loop of model.py:93-96 around
 * DCGRUCell.forward (cell.py:182-210).  h0 may be NULL (zeros).  Rs/Us/Cs/RHs may all be NULL
 * (inference: nothing saved).  Hplanes / RHplanes (each (M-1, T+1, B, N, H); both NULL or both set):
 * the hop rows P_m h_{t-1} (slot t; slot T = P_m h_{T-1}) and P_m (r*h_{t-1}) (slots 0..T-1) that the
 * recurrent kernel forms in LDS anyway, kept as a by-product: the backward need not re-diffuse h and
 * r*h for its weight-gradient GEMMs, and Hplanes + B*N*H (slots 1..T) ARE the input hop planes of the
 * next layer (pass them as its `planes` with d->x_planes_ready = 1, d->x_plane_stride = (T+1)*B*N*H).  ws: eeg_dcrnn_layer_fwd_ws_floats() floats of scratch.
 * Xtm (nullable): when given, X is BATCH-major (B,T,N,Fin) -- the trainer's `input_seq` before
 * model.py:253's transpose -- and Xtm (T,B,N,Fin) receives its time-major copy as a by-product of
 * the diffusion kernel (pass Xtm as X to eeg_dcrnn_layer_bwd); only where
 * eeg_dcrnn_batch_major_ok() returns >= 1.  Where it returns 2, d->x_batch_major = 1 (with Xtm = NULL) consumes
 * the batch-major input without any copy (the diffusion step then moves exactly 4*S*N*F*M bytes). */
size_t eeg_dcrnn_layer_fwd_ws_floats(const eeg_layer_dims* d);
int eeg_dcrnn_batch_major_ok(const eeg_layer_dims* d);
int eeg_dcrnn_layer_fwd(const eeg_layer_dims* d, const float* X, float* Xtm, const float* h0, const float* P,
                        const float* pack, float* planes, float* Hext, float* Rs, float* Us,
                        float* Cs, float* RHs, float* Hplanes, float* RHplanes, float* ws, void* stream);

/* Backward of the same layer (replaces autograd's replay of model.py:93-96 / cell.py).
 * Incoming gradients (each may be NULL): dHseq (T,B,N,H) w.r.t. every h_t; d_at_end (B,N,H) w.r.t.
 * h_{T-1} (the encoder's per-layer final state, model.py:97); d_at_len (B,N,H) w.r.t.
 * h_{lengths[b]-1} (utils.last_relevant_pytorch; lengths int64 (B), NULL -> T).
 * Hplanes / RHplanes: as written by eeg_dcrnn_layer_fwd, or NULL (recomputed here).
 * Outputs: dX (T,B,N,Fin) or NULL; dh0 (B,N,H) or NULL; dWg/dbg/dWc/dbc in reference layout
 * (overwritten).  Reductions are fixed-order: results are run-to-run deterministic. */
size_t eeg_dcrnn_layer_bwd_ws_floats(const eeg_layer_dims* d, int need_dx);
int eeg_dcrnn_layer_bwd(const eeg_layer_dims* d, const float* X, const float* P, const float* pack,
                        const float* planes, const float* Hext, const float* Rs, const float* Us,
                        const float* Cs, const float* RHs, const float* Hplanes, const float* RHplanes,
                        const float* dHseq, const float* d_at_end,
                        const float* d_at_len, const int64_t* lengths, float* dX, float* dh0,
                        float* dWg, float* dbg, float* dWc, float* dbc, float* ws, void* stream);

/* DCGRUDecoder.forward (model.py:160-204): T autoregressive steps through L cells + the projection
 * Linear(H -> Dout), GO symbol = zeros, next input = the projection of step t or, where the HOST
 * array teacher[t] != 0 (curriculum learning, model.py:194-200; NULL = never), targets[t].
 *   targets (T,B,N,Dout) (only read under teacher forcing, may be NULL when teacher is NULL);
 *   h0 (L,B,N,H) encoder finals; packs: HOST array of L device pointers to cell packs
 *   (packs[1..L-1] = the shared cell); Wp (Dout,H), bp (Dout): nn.Linear layout; out (T,B,N,Dout).
 *   saved: eeg_dcrnn_decoder_saved_floats() floats kept for the backward; ws: scratch.
 * The recurrence cannot be hoisted (the input of step t+1 is the output of step t), so the forward
 * launches per step; the backward runs BPTT per step and ALL parameter gradients as GEMMs hoisted
 * over the T steps.  dWg/dbg/dWc/dbc: HOST arrays of L device pointers (entries 1..L-1 equal:
 * gradients of the shared cell are summed); dh0 (L,B,N,H); dWp (Dout,H); dbp (Dout).
 * d->teacher_on_device = 1: `teacher` is a device array (targets must then be given); available where the persistent decoder
 * kernels run (64 units, <= 20 nodes, <= 4 layers, T <= 64, Dout <= 256 with Dout/4 divisible by 4 or 5, where the kernels'
 * LDS tiles fit: past 128 outputs that is up to 5 hop matrices with two layers at Dout <= 200, up to 3 with three layers at
 * Dout <= 256; eeg_dcrnn_decoder_is_persistent answers for a shape), refused elsewhere:
 * the per-step launch sequence is selected by the flags and cannot depend on device memory. */
size_t eeg_dcrnn_decoder_saved_floats(const eeg_decoder_dims* d);
size_t eeg_dcrnn_decoder_fwd_ws_floats(const eeg_decoder_dims* d);
size_t eeg_dcrnn_decoder_bwd_ws_floats(const eeg_decoder_dims* d);
/* d->dropout_p > 0 (model.py:191: `self.projection_layer(self.dropout(output))`, a fresh mask every step): the projection of step t
 * reads mask_t * h_top_t, the recurrence keeps h_top_t.  rng_used = the {seed, offset} pair eeg_dcrnn_rng_take (below) handed out
 * for T*B*N*H/4 counters: element e = ((t*B + b)*N + n)*H + h of the top-layer outputs takes word e%4 of counter offset + e/4.
 * The masks are fused into the persistent kernels (nothing is stored but the dropped rows that dW_p needs) and recomputed in the
 * backward from the same pair.  dropout_p == 0: rng_used may be NULL. */
/* 1 if the persistent decoder kernels cover this shape (then d->teacher_on_device = 1 is available), else 0: the conditions above,
 * both LDS budgets included (e.g. Dout = 200: M = 5, L = 2 yes; M = 5, L = 3 and every M = 7 no). */
int eeg_dcrnn_decoder_is_persistent(const eeg_decoder_dims* d);
int eeg_dcrnn_decoder_fwd(const eeg_decoder_dims* d, const float* targets, const int32_t* teacher,
                          const float* h0, const float* P, const float* const* packs, const float* Wp,
                          const float* bp, const uint64_t* rng_used, float* out, float* saved,
                          float* ws, void* stream);
int eeg_dcrnn_decoder_bwd(const eeg_decoder_dims* d, const int32_t* teacher, const float* P,
                          const float* const* packs, const float* Wp, const float* saved, const float* dOut,
                          const uint64_t* rng_used, float* dh0, float* const* dWg, float* const* dbg,
                          float* const* dWc, float* const* dbc, float* dWp, float* dbp, float* ws, void* stream);

/* Scheduled sampling drawn on the device (model.py:194-200: one `random.random() < teacher_forcing_ratio` per decoder step;
 * utils.py:385-390: ratio = k / (k + exp(batches_seen / k)), k = cl_decay_steps): flags[t] (DEVICE int32[T]) = 1 iff
 * u_t < ratio, u_t = word t%4 of Philox counter offset + t/4 of rng_state (the dropout generator's {seed, offset} pair) / 2^32,
 * evaluated in fp64.  ON THE STREAM: rng_state's offset advances by ceil(T/4) and samples_seen[0] (DEVICE int64, the
 * reference's `step`, train_ssl.py:163,178) by `increment` (the global batch), so every replay of a captured step draws fresh
 * flags against the decayed threshold. */
int eeg_dcrnn_teacher_flags(uint64_t* rng_state, int64_t* samples_seen, int64_t increment, double cl_decay_steps, int T,
                            int32_t* flags, void* stream);

/* eeg_dcrnn_teacher_flags with the increment in device memory: increment[0] (DEVICE int64) is read on the stream -- n_valid of
 * eeg_dcrnn_gather_clips_tail, the real global size of an epoch's short last batch -- so `step += batch_size` stays exact inside a
 * replayed graph. */
int eeg_dcrnn_teacher_flags_dev(uint64_t* rng_state, int64_t* samples_seen, const int64_t* increment, double cl_decay_steps, int T,
                                int32_t* flags, void* stream);

/* Data augmentation drawn on the device (data/dataloader_detection.py:233-256 `_random_reflect`, `_random_scale`, applied per
 * sample at :384-389 in the DataLoader workers).  rng_used = the {seed, offset} pair eeg_dcrnn_rng_take handed out for B
 * counters; clip b uses counter offset + b: word 0's top bit = the reflection coin, word 1 / 2^32 = u, scale = 0.8 + 0.4 u.
 * swap_perm: DEVICE int32[N], the source channel of every node of a reflected clip (data_utils.py:37-62 `get_swap_pairs`).
 * Outputs (DEVICE): flags int32[B]; perm int32[B][N] (swap_perm where flags[b], else the identity) and log_scale float[B]
 * (= log(scale), float) -- the operands of eeg_dcrnn_fft_features; and, when S_out != NULL, the per-clip supports of the
 * distance graph (`_get_combined_graph(swap_nodes)`, :309-333,405-409): S_out[s][b] = flags[b] ? S_reflected[s] : S_plain[s]
 * (S_plain / S_reflected: n_supports x N x N, S_out: n_supports x B x N x N). */
int eeg_dcrnn_augment_draw(const uint64_t* rng_used, int B, int N, const int32_t* swap_perm, int32_t* flags, int32_t* perm,
                           float* log_scale, const float* S_plain, const float* S_reflected, int n_supports, float* S_out,
                           void* stream);

/* Epochs from a data set that stays in device memory: the DataLoader's shuffle and collate (data/dataloader_detection.py:505-523
 * `DataLoader(dataset, shuffle=True, batch_size=...)`; dataloader_classification.py:449-467 and dataloader_ssl.py:441-459 alike: a
 * RandomSampler permutation per epoch, the default collate stacks the samples of a batch).
 *
 * eeg_dcrnn_epoch_keys: keys[i] (DEVICE int64[P], 0 <= key < 2^63) = 63 bits of Philox4x32-10 at counter words (c0, c1, c2, c3) =
 * (i low, i high, epoch, 3) under key `seed` as given.  The generator is that of the dropout masks and augmentation draws, whose
 * draws all run at c2 = c3 = 0 under seeds into which their stream id (0..2) was mixed on the host: the keys are apart from them by
 * the non-zero c3, which is a counter word and not a fourth stream id of that family.  The epoch's permutation is the STABLE argsort
 * of the keys (the caller sorts, once per epoch): a function of (seed, epoch) alone, the same on every rank. */
int eeg_dcrnn_epoch_keys(uint64_t seed, int64_t epoch, int64_t P, int64_t* keys, void* stream);
/* eeg_dcrnn_gather_clips: batch slot b (0 <= b < B) of rank `rank` of `world` takes clip
 *     src = clamp(perm[(cursor[0] + rank*B + b) mod n_perm], 0, P-1)
 * of every pool: x_out[b] = x_pool[src] (rows of x_row_bytes bytes), y_out[b] = y_pool[src] (a second wide tensor, the SSL target;
 * NULL, NULL, 0: none), label_out[b] = label_pool[src] (elements of label_bytes = 4 (float) or 8 (int64) bytes, copied as bits; NULL,
 * NULL, 0: none), len_out[b] = len_pool[src] (int64; both NULL: none).  perm: DEVICE int64[n_perm]; cursor: DEVICE int64[1], read
 * by the launch and advanced by B*world behind it ON THE STREAM (a second, one-thread launch), so a captured step walks through the
 * epoch replay by replay.  The wrap and the clamp are part of the contract: no value of the cursor or of a perm entry makes the
 * kernel touch memory outside the pools (P rows each) and the outputs (B rows each).  Wide rows are whole 16-byte pieces and
 * 16-byte aligned; B*world <= n_perm; outputs must not alias the pools. */
int eeg_dcrnn_gather_clips(const float* x_pool, float* x_out, size_t x_row_bytes, const float* y_pool, float* y_out, size_t y_row_bytes,
                           const void* label_pool, void* label_out, int label_bytes, const int64_t* len_pool, int64_t* len_out,
                           const int64_t* perm, int64_t n_perm, int64_t P, int64_t* cursor, int B, int rank, int world, void* stream);

/* eeg_dcrnn_gather_clips_tail: the gather of an epoch that keeps its short last batch (the reference's DataLoader default,
 * drop_last=False).  The copy, the wrap, the clamp, the two launches and the cursor's advance by B*world are those of
 * eeg_dcrnn_gather_clips: the slots behind the end of the epoch hold real clips.  Three DEVICE outputs, written by the gather launch
 * (in front of the cursor's advance), say which slots count; with pos_b = cursor[0] + rank*B + b, the cursor as it stands:
 *     clip_w[b]  (float[B])  = 1 if 0 <= pos_b < n_perm, else 0
 *     n_valid[0] (int64[1])  = clamp(n_perm - cursor[0], 0, B*world): the clips of the step over ALL ranks
 *     denom[0]   (float[1])  = max(n_valid, 1) / world: the divisor of this rank's criterion (the _w entry points below) -- behind
 *                              the summed all-reduce and its 1/world, sum_valid g_b / denom is the mean over the n_valid clips.
 * A full batch gives clip_w = 1 and denom = B exactly. */
int eeg_dcrnn_gather_clips_tail(const float* x_pool, float* x_out, size_t x_row_bytes, const float* y_pool, float* y_out, size_t y_row_bytes,
                                const void* label_pool, void* label_out, int label_bytes, const int64_t* len_pool, int64_t* len_out,
                                const int64_t* perm, int64_t n_perm, int64_t P, int64_t* cursor, int B, int rank, int world, float* clip_w,
                                float* denom, int64_t* n_valid, void* stream);

/* eeg_dcrnn_gather_records: the sibling of eeg_dcrnn_gather_clips / _tail for clips that are CUT out of whole recordings on the
 * device (the index arithmetic of the reference's loaders at __getitem__ time: `signal_array[:, start:end]`, the SSL target as
 * the head of another clip, the seizure window with its whole 1-s steps and zero padding).  All pointers DEVICE memory.
 *   signals     float32[signal_floats], 16-byte aligned, signal_floats % 4 == 0.  Recording r is channel-major: sample s of channel n
 *               lies at rec_table[r].offset + n * rec_table[r].stride + s.
 *   rec_table   int64[R][3] = (offset, stride, samples), stride >= samples
 *   clip_table  int64[P][4] = (rec, x_start, x_samples, y_start)
 *   label_pool  (P,) elements of label_bytes = 4 / 8 bytes, copied as bits (NULL, NULL, 0: none), as in eeg_dcrnn_gather_clips
 *   perm, n_perm, P, cursor, B, rank, world: the slot arithmetic of eeg_dcrnn_gather_clips,
 *               src = clamp(perm[(cursor[0] + rank*B + b) mod n_perm], 0, P-1); the cursor advances by B*world behind the launch.
 *   N channels, window (% 4 == 0), x_len = Tx * window, y_len = Ty * window floats per channel row (y_len = 0, y_out = NULL: no target)
 * Per batch slot b, with r = clamp(rec, 0, R-1) and keep = (clamp(x_samples, 0, x_len) / window) * window (whole steps only):
 *   x_out[b, n, i] (float[B][N][x_len]) = the sample x_start + i of channel n of recording r if i < keep and 0 <= x_start + i < samples,
 *               else exactly 0.0f;  y_out[b, n, i] (float[B][N][y_len]) the same from y_start over all of y_len
 *   len_out[b]  (int64[B]; NULL: not written) = keep / window
 *   label_out[b] = label_pool[src]
 *   clip_w, denom, n_valid: written exactly as by eeg_dcrnn_gather_clips_tail; all three NULL: the plain form.
 * Bounds are part of the contract: whatever the two tables, perm and the cursor hold, nothing is read outside
 * [signals, signals + signal_floats) -- a sample whose address falls outside it reads as 0.0f -- and nothing is written outside the
 * B output rows, every element of which is written by every launch.  A start with (offset + n*stride + start) % 4 == 0 copies
 * 16-byte pieces; any other start is read as dwords.  The outputs must not alias the signal buffer. */
int eeg_dcrnn_gather_records(const float* signals, int64_t signal_floats, const int64_t* rec_table, int64_t R, const int64_t* clip_table, int64_t P,
                             const void* label_pool, void* label_out, int label_bytes, const int64_t* perm, int64_t n_perm, int64_t* cursor, int B,
                             int rank, int world, int N, int window, int64_t x_len, int64_t y_len, float* x_out, float* y_out, int64_t* len_out,
                             float* clip_w, float* denom, int64_t* n_valid, void* stream);

/* The evaluation pass (train.py:332-431) on the device.
 *
 * eeg_dcrnn_eval_scores: one launch behind the head of every step of a pass over a pool of P clips in order (perm = identity,
 * eeg_dcrnn_gather_clips_tail in front, which has ALREADY advanced the cursor): slot b of logits (B, C) is pool position
 * pos = cursor[0] - B*world + rank*B + b.  A slot writes only if clip_w[b] != 0 AND 0 <= pos < P; whatever the cursor holds,
 * nothing is written outside probs (P, C) and losses (P).  The label is read from label_pool at pos (label_bytes 4: float32
 * {0, 1}, C = 1; 8: int64 classes, C > 1).  Written per slot: C = 1: probs[pos] = sigmoid, losses[pos] = the BCE-with-logits term;
 * C > 1: probs[pos, :] = the float32 softmax row, losses[pos] = the cross-entropy term -- the terms of eeg_dcrnn_bce_logits /
 * eeg_dcrnn_ce_logits on that clip as a batch of one, bit for bit (a class outside 0..C-1: NaN).
 *
 * eeg_dcrnn_eval_metrics: the scores of the pool from probs / labels / losses as ONE record of int64 words in device memory
 * (EEG_EVAL_RECORD_HEAD words, for C > 1 followed by the C x C confusion matrix, row = label, column = prediction); float64 values
 * travel as their bit patterns.  No allocation, no host synchronisation; integer arithmetic and one float64 sum in a fixed
 * order: the record reproduces bit for bit.  P <= EEG_EVAL_MAX_CLIPS.  ws: eeg_dcrnn_eval_metrics_ws_bytes(P, C) bytes (0 for
 * C > 1: ws may be null).  Words (both tasks): 0 n, 9 labels outside {0,1} / 0..C-1, 10 probabilities outside [0,1] or NaN (C > 1:
 * rows holding one), 11 bits of sum(losses).  C = 1 (labels float32): the clips are sorted by (prob, label) (bitonic network, LDS
 * tiles + global steps) and scanned once: 1 n_pos, 2 n_neg, 3 the AUROC numerator sum_v pos(v) * (2 * neg_below(v) + neg(v)) over
 * the distinct values v (AUROC = num / (2 n_pos n_neg)), 4 bits of the threshold used, 5..8 tp, fp, fn, tn of the predictions
 * (double)prob > threshold, 12 search, 13 whether the search found a candidate, 14 / 15 its tp and the bits of its F1.  search != 0:
 * the threshold is the distinct value v whose predictions prob >= v have the largest F1 among those with tp > 0 -- F1 as
 * utils.thresh_max_f1 computes it in float64 from the integer counts, operation for operation, so that candidates whose F1 tie as
 * rationals resolve as they do there -- ties to the lowest v; without a candidate, and with search == 0, it is `thresh`.  C > 1
 * (labels int64): the prediction is the first arg-max of the row. */
#define EEG_EVAL_MAX_CLIPS (1 << 20)
#define EEG_EVAL_RECORD_HEAD 16
int eeg_dcrnn_eval_scores(const float* logits, const void* label_pool, int label_bytes, const float* clip_w, const int64_t* cursor, int B, int C,
                          int rank, int world, int64_t P, float* probs, float* losses, void* stream);
size_t eeg_dcrnn_eval_metrics_ws_bytes(int64_t P, int C);
int eeg_dcrnn_eval_metrics(const float* probs, const void* labels, int label_bytes, const float* losses, int64_t P, int C, int search,
                           double thresh, void* ws, int64_t* record, void* stream);

/* The clustered bootstrap of the evaluator's scores on the device.  A replicate r is a row of int32 counts over G clusters; clip i of
 * cluster groups[i] (int32, 0..G-1; NULL: every clip its own cluster, G = P) weighs counts[r, groups[i]], and every score of the
 * replicate is the weighted form of the score eeg_dcrnn_eval_metrics computes.  Row 0 of the drawn counts is all ones: record 0 is
 * the point estimate.  1 <= G <= EEG_BOOT_MAX_GROUPS, 1 <= n_boot <= EEG_BOOT_MAX_REPLICATES, P <= EEG_EVAL_MAX_CLIPS; counts and
 * records have n_boot + 1 rows.  max_cluster: the clips of the largest cluster as the caller counted them, G * max_cluster < 2^31
 * (a row of drawn counts sums to G, so a replicate's weight fits 31 bits and 2 * W+ * W- fits int64).  A cluster id outside 0..G-1
 * is the caller's to refuse; the kernels count it as cluster 0 and never read outside a counts row.  No allocation, no host
 * synchronisation; integer arithmetic and float64 sums in a fixed order: a record reproduces bit for bit.
 *
 * eeg_dcrnn_boot_counts: counts (n_boot + 1, G).  Row r >= 1 is a multinomial draw of G cluster indices with replacement: draw j is
 * word j % 4 of Philox4x32-10 at the counter words (lo(j / 4), hi(j / 4), r, 4) under key seed (the counter layout of
 * eeg_dcrnn_epoch_keys with a stream word of its own) and names cluster (uint64(word) * G) >> 32; integer atomics in LDS.
 *
 * eeg_dcrnn_boot_detection: probs / labels float32 (P,), losses (P,) float32 or NULL.  ws: eeg_dcrnn_boot_ws_bytes(P) bytes, 8-byte
 * aligned.  One sort per call (64-bit words: the key of eeg_dcrnn_eval_metrics above the clip index, the same bitonic network), one
 * packed 32-bit word per sorted clip (cluster id, label, run start) and the sorted index of the threshold split, then one workgroup
 * per replicate; its counts row sits in LDS for G <= EEG_BOOT_LDS_GROUPS and is read from memory above.  records (n_boot + 1,
 * EEG_BOOT_DET_WORDS) int64: 0 total weight, 1 / 2 weighted positives / negatives, 3 the AUROC numerator sum_v posw(v) * (2 *
 * negw_below(v) + negw(v)) over the runs v of equal probability, 4..7 tp, fp, fn, tn at (double)prob > thresh, 8 the bits of the
 * float64 average precision sum_v posw(v) / W+ * tp(v) / (tp(v) + fp(v)) with tp(v), fp(v) the weights at prob >= v (NaN without a
 * positive), 9 the bits of the float64 sum_i w_i * loss_i in pool order (0 without losses).
 *
 * eeg_dcrnn_boot_classification: probs (P, C) float32, labels int64, 2 <= C <= EEG_BOOT_MAX_CLASSES; records (n_boot + 1, C * C) int64
 * weighted confusion matrices (row = label, column = the first arg-max; a row eeg_dcrnn_eval_metrics counts as bad is left out).
 *
 * eeg_dcrnn_boot_records: records[r, k] = sum_g counts[r, g] * rec_records[g, k] for rec_records (G, K) int64 (one integer record per
 * cluster, e.g. the rec_records of eeg_dcrnn_event_scores), 1 <= K <= EEG_BOOT_MAX_RECORD_WORDS, int64 arithmetic modulo 2^64. */
#define EEG_BOOT_MAX_GROUPS (1 << 20)
#define EEG_BOOT_MAX_REPLICATES 65535
#define EEG_BOOT_DET_WORDS 10
#define EEG_BOOT_MAX_CLASSES 32
#define EEG_BOOT_MAX_RECORD_WORDS 64
#define EEG_BOOT_LDS_GROUPS 32768
int eeg_dcrnn_boot_counts(uint64_t seed, int64_t G, int64_t n_boot, int32_t* counts, void* stream);
size_t eeg_dcrnn_boot_ws_bytes(int64_t P);
int eeg_dcrnn_boot_detection(const float* probs, const float* labels, const int32_t* groups, const float* losses, int64_t P, int64_t G,
                             int64_t max_cluster, const int32_t* counts, int64_t n_boot, double thresh, void* ws, int64_t* records, void* stream);
int eeg_dcrnn_boot_classification(const float* probs, const int64_t* labels, const int32_t* groups, int64_t P, int C, int64_t G, int64_t max_cluster,
                                  const int32_t* counts, int64_t n_boot, void* ws, int64_t* records, void* stream);
int eeg_dcrnn_boot_records(const int64_t* rec_records, int64_t G, int K, const int32_t* counts, int64_t n_boot, int64_t* records, void* stream);

/* The SSL evaluation pass (train_ssl.py:232-280) on the device.
 *
 * eeg_dcrnn_ssl_eval_scores: one launch behind the decoder of every step of a pass over a pool of P clips in order, the twin of
 * eeg_dcrnn_eval_scores (same slot arithmetic, unsigned: pos = cursor[0] - B*world + rank*B + b; a slot writes only if
 * clip_w[b] != 0 AND 0 <= pos < P; nothing is ever written outside scores and keep).  pred / target: (B, clip_elems) float32, the
 * batch as the loss sees it (standardised), 16-byte aligned, clip_elems a multiple of D, D a multiple of 4,
 * clip_elems < EEG_SSL_EVAL_MAX_CLIP_ELEMS.  Per element the terms of eeg_dcrnn_masked_loss: scaled != 0: ps = p*std + mean,
 * ys = y*std + mean (two roundings each), d = ps - ys in float32, masked in iff ys != mask_val.  scores is (3, P) float64:
 * scores[0][pos] = the float64 sum of the float32 |d| over the clip's masked-in elements with a finite d, scores[1][pos] = the
 * number of masked-in elements, scores[2][pos] = the number of masked-in elements whose d is NaN or infinite.  One workgroup per
 * slot, a fixed assignment of 16-byte pieces to threads and a fixed tree: a clip's sum has the same bits whatever B, slot, rank.
 * keep: null, or (P, clip_elems) float32, 16-byte aligned: the slot's pred is copied to keep[pos].
 *
 * eeg_dcrnn_ssl_eval_metrics: the pass's record from scores, EEG_SSL_EVAL_RECORD_WORDS float64 words in device memory, one block,
 * fixed order: 0 n = P, 1 batches = ceil(P / G), 2 loss = sum_g n_g * L_g / P over the consecutive groups g = [g*G, min((g+1)*G, P))
 * with L_g = S_g / C_g (0 where C_g == 0): the reference's AverageMeter over batches of G clips, 3 pool_mae = sum abs_sum / sum
 * count (0 if nothing is masked in), 4 / 5 / 6 the totals of abs_sum, count and bad, 7 the groups with C_g == 0.  G >= 1; a G
 * above P is one group.  No allocation, no host synchronisation. */
#define EEG_SSL_EVAL_MAX_CLIP_ELEMS (1 << 24)
#define EEG_SSL_EVAL_RECORD_WORDS 8
int eeg_dcrnn_ssl_eval_scores(const float* pred, const float* target, const float* clip_w, const int64_t* cursor, int B, int64_t clip_elems, int D,
                              int rank, int world, int64_t P, int scaled, float mean, float std, float mask_val, double* scores, float* keep,
                              void* stream);
int eeg_dcrnn_ssl_eval_metrics(const double* scores, int64_t P, int64_t G, double* record, void* stream);

/* The fit of the input scaler on the device: the scalar mean and std of the UN-standardised model inputs over a pool of P clips (the
 * reference's StandardScaler, whose two numbers it reads from files made offline), without writing the inputs.
 *
 * eeg_dcrnn_feature_moments: one call behind the gather of every step of a pass over the pool in order.  raw: the gathered batch
 * (B, N, T*W) float32, 16-byte aligned.  kind 0: the values of clip b are the float32 numbers eeg_dcrnn_fft_features writes to
 * feat_raw for it without augmentation (W % 4 == 0, W/4 + 1 <= 64; W = 200: the mixed-radix transform, else the direct DFT), bit
 * for bit, never stored.  kind 1: the float32 samples as given (W % 4 == 0) -- the time-domain windows; ready features (B, T, N, D)
 * go in as N = 1, W = N*D.  lengths: null, or int64 (B): clip b counts its first clamp(lengths[b], 1, T) steps only.  scores is
 * (4, P) float64: sum | sumsq | count | bad of the clip at each pool position: every finite value v adds (double)v and
 * (double)v * (double)v and 1 to count, a NaN or infinite value 1 to bad.  Slot arithmetic and bound of eeg_dcrnn_ssl_eval_scores
 * (unsigned: pos = cursor[0] - B*world + rank*B + b; a slot writes only if clip_w[b] != 0 AND 0 <= pos < P; clip_w null: every slot
 * counts; cursor null: pos = rank*B + b); nothing is written outside scores and ws.  No floating-point atomics: fixed per-thread
 * order, a fixed tree per workgroup, the chunks of a clip added in chunk order from ws (eeg_dcrnn_moments_ws_bytes(B, N, T, W, kind)
 * bytes, 8-byte aligned; 0: the shape is refused).  The partition depends on (N, T, W, kind) alone: a clip's four words have the same
 * bits whatever B, slot, rank, cursor and length.  B <= EEG_MOMENTS_MAX_BATCH, N*T*W < 2^31, P <= EEG_EVAL_MAX_CLIPS.
 *
 * eeg_dcrnn_moments_record: the pool's record from scores, EEG_MOMENTS_RECORD_WORDS float64 words in device memory, one block, an
 * order that depends on P alone: 0 clips = positions with count > 0, 1 count, 2 sum, 3 sumsq, 4 mean = sum / count, 5 std =
 * sqrt(sumsq / count - mean^2) (the population std; every operation rounded on its own), 0 where that variance is at or below
 * 2^-50 * sumsq -- inside the rounding of the sums, negative values among them: a pool of equal values reports std = 0 --, 6 bad;
 * count == 0: mean = std = 0.  No allocation, no host synchronisation. */
#define EEG_MOMENTS_RECORD_WORDS 7
#define EEG_MOMENTS_MAX_BATCH 65535
size_t eeg_dcrnn_moments_ws_bytes(int B, int N, int T, int W, int kind);
int eeg_dcrnn_feature_moments(const float* raw, int B, int N, int T, int W, int kind, const int64_t* lengths, const float* clip_w,
                              const int64_t* cursor, int rank, int world, int64_t P, void* ws, double* scores, void* stream);
int eeg_dcrnn_moments_record(const double* scores, int64_t P, double* record, void* stream);

/* Whole recordings behind the detection head: a scan's per-bin timeline, seizure events from it, their scores.  A bin is one step of
 * `window` samples.  R recordings; recording r owns the bins bin_off[r] .. bin_off[r+1] (int64 (R+1): prefix sums of the recordings'
 * whole steps, total_bins = bin_off[R] < 2^31) of every flat per-bin buffer, and the rows clip_off[r] .. clip_off[r+1] (int64 (R+1)) of
 * the clip table (int64 (P, 4) = (rec, x_start, x_samples, y_start), eeg_dcrnn_gather_records), whose rows start at ascending whole steps
 * within a recording and are x_steps steps long.  All pointers are device memory.  No allocation, no host synchronisation, no atomics,
 * every float sum in ascending index order; EVERY output element is written by EVERY launch, and every index derived from a table is
 * clamped: whatever the tables hold, nothing is read or written outside the buffers as sized here.
 *
 * eeg_dcrnn_scan_timeline: probs (P) float32, one per table row -> timeline (total_bins) float32, cover (total_bins) int32.  Bin j of
 * recording r is covered by the rows of r with start_step <= j < start_step + x_steps (start_step = x_start / window, read from the
 * table; found by binary search: a gather).  agg 0: the float32 sum of the covering probabilities in ascending row order, divided by
 * float(cover); agg 1: their maximum; an uncovered bin: value 0, cover 0.
 *
 * eeg_dcrnn_scan_events: per recording over its bins 0 .. S-1, one workgroup each, the bins streamed through LDS in chunks of
 * EEG_SCAN_CHUNK_BINS: q_j = the float32 ascending sum of timeline_i over the COVERED i in [j-h, j+h] and [0, S), over their number,
 * h = (smooth_bins - 1) / 2 (smooth_bins odd, 1 .. EEG_SCAN_MAX_SMOOTH_BINS; an uncovered j: 0) -> smoothed (total_bins); state_j = on
 * if q_j >= th_on, off if q_j < th_off or j is uncovered, else state_{j-1} (state_{-1} off; th_off <= th_on); maximal runs of on are
 * events [a, b); a run at most merge_gap off bins behind the event before it is merged into it (left to right, chains; 0 merges
 * nothing); events shorter than min_bins are then dropped.  events (R, E_max, 2) int32 = (onset, offset exclusive) in order, zero rows
 * behind them; event_count (R) int32 = the TRUE number of events of the recording, which may exceed E_max: such rows are not written.
 *
 * eeg_dcrnn_event_scores: events / event_count as above, ref (R, A_max, 2) int32 half-open reference intervals in bins, ref_count (R)
 * int32 -> rec_records (R, EEG_SCAN_RECORD_WORDS) int64 per recording and record (EEG_SCAN_RECORD_WORDS) int64, their word-wise sum:
 * 0 n_ref, 1 n_hyp = min(event_count, E_max), 2 ref_hit: reference events sharing a bin with a detected event, 3 hyp_hit: detected
 * events sharing a bin with a reference event, 4 covered_bins, 5..8 tp, fp, fn, tn over the covered bins (positive inside a reference
 * interval, predicted inside a detected event), 9 overflowed: recordings with event_count > E_max. */
#define EEG_SCAN_CHUNK_BINS 2048
#define EEG_SCAN_MAX_SMOOTH_BINS 129
#define EEG_SCAN_RECORD_WORDS 10
#define EEG_SCAN_MAX_RECORDINGS (1 << 20)
int eeg_dcrnn_scan_timeline(const float* probs, int64_t P, const int64_t* clip_table, const int64_t* clip_off, const int64_t* bin_off, int64_t R,
                            int64_t total_bins, int x_steps, int window, int agg, float* timeline, int32_t* cover, void* stream);
int eeg_dcrnn_scan_events(const float* timeline, const int32_t* cover, const int64_t* bin_off, int64_t R, int64_t total_bins, int smooth_bins,
                          float th_on, float th_off, int merge_gap, int min_bins, int E_max, float* smoothed, int32_t* events, int32_t* event_count,
                          void* stream);
int eeg_dcrnn_event_scores(const int32_t* events, const int32_t* event_count, int E_max, const int32_t* ref, const int32_t* ref_count, int A_max,
                           const int32_t* cover, const int64_t* bin_off, int64_t R, int64_t total_bins, int64_t* record, int64_t* rec_records,
                           void* stream);

/* Native-rate recordings to the model's rate on the device: the Fourier resampling of whole recordings (the reference's offline step,
 * data/resample_signals.py:38-43 -> data/data_utils.py:158-170 `resampleData` = scipy.signal.resample over the whole recording, on the
 * float64 signals of `getEDFsignals`).  Per channel row x of n_in samples, in float64:
 *   X = rfft(x);  N = min(n_out, n_in);  Y[0 .. N/2] = X[0 .. N/2], zero above;  N even: Y[N/2] *= 2 (n_out < n_in) or 0.5 (n_in < n_out);
 *   y = irfft(Y, n_out) * n_out / n_in, rounded once to float32 on the store.
 * Any lengths (prime ones included): both transforms are chirp-z transforms on power-of-two float64 complex FFTs of M1 >= n_in + N/2
 * and M2 >= n_out/2 + n_out points (csrc/kernels_resample.h).  No atomics, a fixed order of operations: a channel's output bits depend
 * on that channel's samples and (n_in, n_out) alone -- not on the channel count, the chunking or what the workspace held.
 *
 * eeg_dcrnn_resample: in (channels rows of n_in samples, row c at in + c * in_stride elements; float32, or float64 with in_f64 = 1)
 * -> out + c * out_stride .. + n_out float32; nothing else of out is written (padding behind a row keeps its bits).  2 <= n_in <=
 * EEG_RESAMPLE_MAX_SAMPLES, 1 <= n_out <= EEG_RESAMPLE_MAX_SAMPLES, strides >= the lengths.  ws: 16-byte aligned device memory of
 * ws_bytes; eeg_dcrnn_resample_ws_bytes(n_in, n_out, channels) runs all channels at once, anything down to
 * eeg_dcrnn_resample_ws_bytes(n_in, n_out, 1) runs them in chunks with the same bits (what bounds the memory of an hour-long
 * recording); less is refused.  eeg_dcrnn_resample_ws_bytes returns 0 for a shape the call would refuse. */
#define EEG_RESAMPLE_MAX_SAMPLES (1ll << 22)
size_t eeg_dcrnn_resample_ws_bytes(int64_t n_in, int64_t n_out, int channels);
int eeg_dcrnn_resample(const void* in, int in_f64, int channels, int64_t n_in, int64_t in_stride, int64_t n_out, float* out, int64_t out_stride,
                       void* ws, size_t ws_bytes, void* stream);

/* EDF recordings decoded on the device: the int16 payload of an EDF file -> the physical signals of the selected channels (the
 * reference's `getEDFsignals`, data/data_utils.py, through EDFlib's readSignal).  The payload (everything behind the header) lies in
 * device memory as it is in the file: num_records records of R little-endian int16 each; selected channel c has n samples per record,
 * the first at int16 index chan_off[c] of the record.  Per sample, in float64,
 *   out[c * out_stride + r * n + j] = gain[c] * (offset[c] + (double)payload_i16[r * R + chan_off[c] + j])
 * with gain = (pmax - pmin) / (dmax - dmin), offset = pmax / gain - dmax computed by the caller (EDFlib's arithmetic): one correctly
 * rounded add, then one correctly rounded multiply; out_f64 = 0 rounds that value once to float32.  chan_off / gain / offset are HOST
 * arrays of `channels` entries; they travel in the kernel argument (no device table, no copy).  One launch, no workspace, no atomics;
 * nothing outside the payload's num_records * R int16 is read (a lane reads the two bytes of its own sample only, at any parity of R,
 * chan_off and the payload address) and nothing outside the `channels` rows of num_records * n elements is written.
 * Refused, naming the argument: null pointers, an odd payload address, channels outside 1..EEG_EDF_MAX_CHANNELS, num_records < 1,
 * n outside 1..2^30, payload_bytes < 2 * num_records * R, chan_off[c] + n > R (or a negative chan_off), out_stride < num_records * n,
 * out not aligned to its element. */
#define EEG_EDF_MAX_CHANNELS 32
int eeg_dcrnn_edf_decode(const void* payload, size_t payload_bytes, int64_t num_records, int64_t R, int64_t n, int channels, const int64_t* chan_off,
                         const double* gain, const double* offset, int out_f64, void* out, int64_t out_stride, void* stream);

/* Occlusion maps on the device: group g of channels of clip b is overwritten with `fill` over the window of steps [t0, t0 + w) and the
 * map records how far the predicted probability drops.  All variants of a window start from the unoccluded clip's state at t0.
 *
 * eeg_dcrnn_occlude_expand: one launch per window builds what the layer entry points need for its B * G variants, v = b * G + g,
 * into buffers the caller owns.  x (B, T, N, D) float32, batch-major; hext: a HOST table of L <= EEG_OCCLUDE_MAX_LAYERS device
 * pointers, the `hext` (T+1, B, N*H) of every encoder layer of the unoccluded pass (slot t = the state in front of step t);
 * groups (G, N) int32 0/1 in device memory, 1 <= G <= EEG_OCCLUDE_MAX_GROUPS (an empty group occludes nothing); lengths: device
 * int64 (B) or NULL.  Written:
 *   x_var   (T - t0, B*G, N, D)  time-major: `fill` where step s < w and groups[g][n] != 0, else x[b][t0 + s][n][:]
 *   h0_var  (L, B*G, N*H)        hext[l][t0][b][:] for every g
 *   len_var (B*G) int64          max(lengths[b] - t0, 1); lengths NULL: T - t0
 * and nothing else.  D % 4 == 0, N*H % 4 == 0, x / hext / x_var / h0_var 16-byte aligned (the rows move as 16-byte pieces, bit for bit).
 *
 * eeg_dcrnn_occlusion_scores: one launch per window behind the head.  var_logits (B*G, C), base_logits (B, C) float32;
 * maps (B, Tw, G) float32: maps[b][k][g] = p_b - p_{b,k,g}, exactly 0.0f where the window starts at or behind the clip's end
 * (t0 >= lengths[b]; lengths NULL: never).  C == 1: p = sigmoid(logit); C > 1: p = softmax(logits)[cls_b] with cls_b = target[b]
 * CLAMPED to 0..C-1, or (target NULL) the arg-max of the baseline row, lowest index on ties.  The probabilities are evaluated in
 * double from the float32 logits and the difference is rounded to float32 once.  k == 0 also writes base_prob[b] = p_b and
 * (target_out nullable, int64 (B)) the class followed. */
#define EEG_OCCLUDE_MAX_LAYERS 4
#define EEG_OCCLUDE_MAX_GROUPS 64
int eeg_dcrnn_occlude_expand(const float* x, const float* const* hext, int L, const int32_t* groups, const int64_t* lengths, int B, int T, int N, int D,
                             int H, int G, int t0, int w, float fill, float* x_var, float* h0_var, int64_t* len_var, void* stream);
int eeg_dcrnn_occlusion_scores(const float* var_logits, const float* base_logits, const int64_t* lengths, const int64_t* target, int B, int G, int C,
                               int Tw, int k, int t0, float* maps, float* base_prob, int64_t* target_out, void* stream);

/* utils.last_relevant_pytorch (utils.py:346-357): last[b] = Htop[lengths[b]-1, b]. Htop (T,B,NH). */
int eeg_dcrnn_gather_last(const float* Htop, const int64_t* lengths, int T, int B, int NH,
                          float* last, void* stream);
/* The generator behind the fused dropout masks (nn.Dropout of model.py:191,267): Philox4x32-10, state = device uint64[2]
 * {seed, offset}.  rng_take copies the pair to rng_used (device uint64[2]) and advances the state's offset by `groups` counters --
 * ON THE STREAM, so a replayed HIP graph draws fresh masks every time.  A forward entry point that drops is handed rng_used and
 * keeps element e of its dropped tensor iff word e%4 of counter offset + e/4 under key seed is >= p * 2^32, scaled by 1/(1-p);
 * nothing is stored, the backward entry point recomputes the mask from the same pair. */
int eeg_dcrnn_rng_take(uint64_t* rng_state, uint64_t groups, uint64_t* rng_used, void* stream);
/* model.py:267-270: logits[b][c] = max_n fc(relu(dropout(z[b][n]))); arg[b][c] = maximising node.
 * dropout_p = nn.Dropout's p while the module is training (README.md:83 trains the 4-class model with --dropout 0.5), else 0;
 * dropout_p > 0: rng_used = the pair rng_take handed out for B*N*H/4 counters (NULL allowed otherwise). */
int eeg_dcrnn_cls_head_fwd(const float* z, const float* W, const float* bias, int B, int N, int H,
                           int C, float dropout_p, const uint64_t* rng_used,
                           float* logits, int32_t* arg, void* stream);
int eeg_dcrnn_cls_head_bwd(const float* z, const float* W, const float* dlogits, const int32_t* arg,
                           int B, int N, int H, int C, float dropout_p, const uint64_t* rng_used,
                           float* dz, float* dW, float* dbias, void* stream);

/* Head + criterion + their backward for the optimisation step (model.py:260-270 forward, train.py:203-206,266-272 loss and the
 * head's share of `loss.backward()`), two launches: logits (B,C), arg (B,C) as eeg_dcrnn_cls_head_fwd; loss[0] = mean criterion,
 * kind 0 = nn.BCEWithLogitsLoss (C == 1, targets float[B]), kind 1 = nn.CrossEntropyLoss (targets int64[B]; a label outside
 * 0..C-1 makes the loss NaN); dlogits (B,C) = d loss / d logits; dz (B,N,H) = d loss / d z (the seed of the encoder's backward);
 * dW (C,H), dbias (C) = the gradients of the fc layer (overwritten).  Sums over the batch run in a fixed order.
 * ws: eeg_dcrnn_cls_head_loss_ws_floats(B, H, C) floats. */
size_t eeg_dcrnn_cls_head_loss_ws_floats(int B, int H, int C);
int eeg_dcrnn_cls_head_loss(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N,
                            int H, int C, float dropout_p, const uint64_t* rng_used, float* logits, int32_t* arg,
                            float* dlogits, float* dz, float* dW, float* dbias, float* loss, float* ws, void* stream);
/* eeg_dcrnn_cls_head_loss over the clips that count: clip_w (DEVICE float[B]) and denom (DEVICE float[1]) as written by
 * eeg_dcrnn_gather_clips_tail.  The mean divides by denom[0] instead of B; a clip with clip_w[b] == 0 is selected out (not
 * multiplied): dlogits = 0 and dz = 0 for it, nothing from it in dW, dbias and loss -- a cross-entropy label outside 0..C-1 there
 * does not make the loss NaN (on a clip that counts it does) -- while logits and arg are written for every clip.  Same launches and
 * order of sums: clip_w = 1 and denom = B give the results of eeg_dcrnn_cls_head_loss bit for bit. */
int eeg_dcrnn_cls_head_loss_w(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N,
                              int H, int C, float dropout_p, const uint64_t* rng_used, const float* clip_w, const float* denom,
                              float* logits, int32_t* arg, float* dlogits, float* dz, float* dW, float* dbias, float* loss, float* ws,
                              void* stream);
/* mask[e] = keep(e) / (1 - p) for e < n: the factors the fused kernels apply for the {seed, offset} pair in rng_used (a forward
 * call's output), materialised -- the parity tests hand them to the oracle. */
int eeg_dcrnn_dropout_mask(const uint64_t* rng_used, size_t n, float dropout_p, float* mask, void* stream);

/* Losses that seed backward (train.py:203-206,266-268), value + gradient in one launch:
 * nn.BCEWithLogitsLoss() on logits (B,) / nn.CrossEntropyLoss() on logits (B,C); loss[0] = mean. */
int eeg_dcrnn_bce_logits(const float* logits, const float* y, int B, float* loss, float* dlogits, void* stream);
int eeg_dcrnn_ce_logits(const float* logits, const int64_t* y, int B, int C, float* loss, float* dlogits,
                        void* stream);
/* utils.compute_regression_loss (utils.py:431-495; train_ssl.py:165-170) on n elements: optional
 * scalar StandardScaler inverse transform v*std + mean of both tensors, mask = (y_true != mask_val),
 * kind 0: masked MAE (loss_fn == 'mae'); kind 1: `masked_mse_loss`, which returns the masked RMSE
 * (what train_ssl.py's "MAE" string actually selects).  loss[0] = value; dpred (nullable) = gradient
 * w.r.t. pred.  ws: eeg_dcrnn_masked_loss_ws_floats() floats. */
size_t eeg_dcrnn_masked_loss_ws_floats(void);
int eeg_dcrnn_masked_loss(const float* pred, const float* y, size_t n, int use_scaler, float mean, float std_,
                          float mask_val, int kind, float* loss, float* dpred, float* ws, void* stream);
/* The three criteria over the clips that count (clip_w DEVICE float[B], denom DEVICE float[1]: eeg_dcrnn_gather_clips_tail).
 * bce / ce: as eeg_dcrnn_cls_head_loss_w -- selection, mean over denom[0].  masked_loss_w: pred / y are B clips of n / B elements
 * each (n % B == 0), the mask is (y != mask_val) && clip_w[clip] != 0, L = the masked MAE / RMSE over it, and the rank's factor
 * f = (sum_b clip_w[b]) / denom[0] goes on both outputs: loss[0] = f * L, dpred = f * dL/dpred (no element left: 0 and 0).
 * With clip_w = 1 and denom = B all three equal their unweighted entry points bit for bit. */
int eeg_dcrnn_bce_logits_w(const float* logits, const float* y, int B, const float* clip_w, const float* denom, float* loss,
                           float* dlogits, void* stream);
int eeg_dcrnn_ce_logits_w(const float* logits, const int64_t* y, int B, int C, const float* clip_w, const float* denom, float* loss,
                          float* dlogits, void* stream);
int eeg_dcrnn_masked_loss_w(const float* pred, const float* y, size_t n, int B, const float* clip_w, const float* denom, int use_scaler,
                            float mean, float std_, float mask_val, int kind, float* loss, float* dpred, float* ws, void* stream);
/* Class and sample weights.  The criteria with a MULTIPLIER per clip: clip_u (DEVICE float[B], every u_b >= 0) and denom (DEVICE
 * float[1]) as written by eeg_dcrnn_clip_weights; loss[0] = (sum_b u_b * l_b) / denom[0], dlogits = (u_b * g_b) / denom[0] with l_b,
 * g_b the clip's own criterion term and its gradient (hence dz, dW, dbias of the head).  u_b = w[y_b], denom = sum_b u_b is
 * nn.CrossEntropyLoss(weight=w); u_b = y_b ? p : 1, denom = B is nn.BCEWithLogitsLoss(pos_weight=p) on 0/1 labels.  u_b == 0 selects
 * the clip out as clip_w == 0 does in the _w entry points (its label is not looked at; logits and arg are still written).  Same
 * launches and order of sums: clip_u = 1 and denom = B give the unweighted results bit for bit. */
int eeg_dcrnn_cls_head_loss_cw(const float* z, const float* W, const float* bias, const void* targets, int kind, int B, int N,
                               int H, int C, float dropout_p, const uint64_t* rng_used, const float* clip_u, const float* denom,
                               float* logits, int32_t* arg, float* dlogits, float* dz, float* dW, float* dbias, float* loss, float* ws,
                               void* stream);
int eeg_dcrnn_bce_logits_cw(const float* logits, const float* y, int B, const float* clip_u, const float* denom, float* loss,
                            float* dlogits, void* stream);
int eeg_dcrnn_ce_logits_cw(const float* logits, const int64_t* y, int B, int C, const float* clip_u, const float* denom, float* loss,
                           float* dlogits, void* stream);
/* The multipliers of one step and their divisor, one launch of one workgroup, plain stores at fixed addresses (capturable):
 *   u = valid * class_w[class(label)] * sample_w[src]      (class_w DEVICE float[C] or NULL with C = 0; sample_w DEVICE float[P] or NULL)
 * class(label) = the int64 label (label_bytes 8; outside 0..C-1: weight 1) or label >= 0.5 ? 1 : 0 (label_bytes 4: detection's float
 * labels, taken to be 0 or 1; C == 2).  clip_u[b] for this rank's B slots; denom[0] = D / world with norm 0: D = the sum of u over
 * ALL slots of the step (a zero sum: D = 1), norm 1: D = max(number of valid slots, 1) -- behind the summed all-reduce and its
 * 1 / world the gradient is sum u g / D.  The sum is float64 in a fixed order, rounded once.
 * Sampler form (perm != NULL): labels is the label POOL (P entries), slot s of the step's B * world is the clip of
 * eeg_dcrnn_gather_clips at position (cursor[0] - back) + s of perm (same wrap, clamp and validity rule as
 * eeg_dcrnn_gather_clips_tail); back = 0 in front of the step's gather, B * world behind it (the gather has advanced the cursor).
 * Every rank computes the same divisor bits from its own copy of the pool: no communication.
 * Batch form (perm == NULL; cursor, sample_w NULL, back 0): labels are the batch's own B labels, every slot is valid and the divisor
 * is the rank's own (world is taken as 1: data-parallel, the mean of the ranks' weighted means). */
int eeg_dcrnn_clip_weights(const void* labels, int label_bytes, const int64_t* perm, int64_t n_perm, int64_t P, const int64_t* cursor,
                           int64_t back, int B, int rank, int world, const float* class_w, int C, const float* sample_w, int norm,
                           float* clip_u, float* denom, void* stream);
/* clip_grad_norm_(max_norm) + torch.optim.Adam(lr, betas, eps, weight_decay = coupled L2) step
 * `step` (1-based) over flat fp32 buffers of n elements (train.py:222-223,273-275).  grads are
 * first multiplied by grad_scale (1/world_size after a summed all-reduce).  ws: 64 floats scratch;
 * norm_out (nullable) receives the pre-clip gradient norm.  Deterministic (fixed-order sums). */
size_t eeg_dcrnn_clip_adam_ws_floats(void);
int eeg_dcrnn_clip_adam(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                        float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int step, float grad_scale, float* ws, float* norm_out, void* stream);

/* The same update with the optimiser's step count and learning rate in DEVICE memory: step_dev[0] (int32, the number of updates
 * applied so far) is incremented on the stream and the bias corrections 1 - beta^step are formed in the kernel; lr_dev[0] is the
 * current learning rate (the host rewrites it between epochs, train.py:224,329 cosine schedule).  With these two the whole
 * optimisation step -- zero_grad ... backward, [all-reduce], clip, Adam -- is capturable as ONE HIP graph. */
int eeg_dcrnn_clip_adam_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                            float max_norm, const float* lr_dev, float beta1, float beta2, float eps,
                            float weight_decay, int32_t* step_dev, float grad_scale, float* ws, float* norm_out,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEG_DCRNN_H */
