/* mmego_hip.h -- C ABI of libmmego_hip.so: the MI355X (gfx950) kernels behind the mmEgo hot path.
 *
 * The reference (yenanjing/mmEgo) has no FFI of its own: its boundary is the Python nn.Module
 * interface (Net/IMU_Net.py, Net/Upper_Net.py, Net/Lower_Net.py, Net/GCN.py) and the train_once bodies
 * of Processor/Train/Train_*.py.  This library sits one level below that boundary; each entry point
 * names the chain of aten ops of the reference it replaces.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (the library never allocates or frees);
 *  - `stream` is a hipStream_t (pass the stream the caller's tensors are ordered on); all calls are
 *    asynchronous and capturable into a HIP graph (no allocation, no synchronisation inside);
 *  - tensors are fp32, row-major "rows x channels" (channels-last); `ld*` / `s*` are ELEMENT strides;
 *  - return value: 0 = ok, -1 = bad argument, >0 = hipError_t of the failed launch;
 *  - re-entrant per stream; workspaces are passed in by the caller.
 */
#ifndef MMEGO_HIP_H
#define MMEGO_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense products (gemm.hip) ---------------------------------------------------------------
 * C[b](m,n) (+)= sum_k A[b](m,k) * B[b](k,n) (+ bias[n]) (relu).  A(m,k) = A[m*sam + k*sak + b*sAb],
 * B(k,n) = B[k*sbk + n*sbn + b*sBb], C(m,n) = C[m*scm + n*scn + b*sCb].  nsplit > 1 splits K into slabs
 * in `splitk_ws` (nsplit*nbatch*M*N floats) that are then summed in a fixed order (deterministic).
 * Order of the epilogue, the same in every kernel and in the split-K reducer:
 *   C = cmulop( C_old + relu( sum_k A B + bias ) )
 * -- bias first, then ReLU (relu == 1 only), then the old C is added (accumulate == 1 only: the ReLU does NOT cover it), then cmul
 * (relu 0 / 1: times cmul; relu == 2: 0 where cmul <= 0).  accumulate == 2 (nsplit > 1, nbatch == 1, no bias, no relu): the slabs stay
 * in splitk_ws for the caller to sum and C is not written.
 * Replaces: nn.Linear / Conv1d(k=1) / Conv2d(1x1, 9x1) / Conv3d forward and their weight/input
 * gradients -- Net/Upper_Net.py:242-301,343-364, Net/Lower_Net.py:40-72,95-123, Net/GCN.py:46-60,
 * and the LSTM input projections of Net/IMU_Net.py:58-62. */
/* (sBiasb: element stride of `bias` between batches, 0 = one bias for all -- lets the two directions' input projections of a
 * BiLSTM layer run as ONE batched product: same A, two weight / bias / output-column blocks.)
 * cmul (may be NULL; nsplit == 1 only): elementwise multiplier in C's layout applied after bias / relu / accumulate -- the
 * inter-layer dropout mask on an LSTM layer's input gradient.  relu == 2 (with cmul): no ReLU on the result; instead the result is
 * set to 0 where cmul <= 0 -- ReLU's backward on an input gradient, cmul = the layer's forward output (Upper_Net.py:350-351).
 * asum (may be NULL): asum[b*M + m] (+)= sum_k A[b](m,k), computed from the operand values the product loads anyway -- the bias
 * gradient beside a weight gradient dW = dY^T X (A = dY^T).  Only for the small-product shapes (about M*N*nsplit*nbatch <=
 * 2 M outputs, K slabs >= 64: bad argument otherwise); with nsplit > 1 splitk_ws needs nsplit*nbatch*M more floats. */
int mmego_gemm(void* stream, const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C,
               long scm, long scn, const float* bias, int M, int N, int K, int nbatch, long sAb, long sBb, long sCb,
               int relu, int accumulate, float* splitk_ws, int nsplit, long sBiasb, const float* cmul, float* asum);
/* Several INDEPENDENT products in one launch: each entry is one mmego_gemm argument set.  When all of them are small-tile products
 * of one operand orientation (what mmego_gemm would hand to its K-quartered kernel, unsplit), they share a launch -- grid.z is cut
 * into the products' ranges --; otherwise they run as n mmego_gemm calls in order.  Same results either way; an entry whose options
 * mmego_gemm refuses (null A / B / C, a size < 1, relu outside 0..2 or 2 without cmul, accumulate == 2 on an unsplit, batched, biased
 * or relu product, cmul or sBiasb with nsplit > 1) makes the call a bad argument before any entry is launched.  For the leaf
 * products of a backward pass (weight gradients of a BiLSTM stack: the reference's autograd computes them per parameter, e.g.
 * Net/Upper_Net.py:333), which otherwise sit one behind the other in a dependent chain of small kernels. */
typedef struct MmegoGemmDesc {
  const float* A; long sam, sak;
  const float* B; long sbk, sbn;
  float* C; long scm, scn;
  const float* bias;
  int M, N, K, nbatch;
  long sAb, sBb, sCb;
  int relu, accumulate;
  float* splitk_ws; int nsplit;
  long sBiasb;
  const float* cmul; float* asum;
} MmegoGemmDesc;
int mmego_gemm_group(void* stream, int n, const MmegoGemmDesc* descs);

/* ---- BatchNorm and row-wise helpers (bn.hip) ----------------------------------------------------
 * Train-mode statistics of X[rows, C] (+ running-stat update with torch semantics: momentum, unbiased
 * running var) -> mean, invstd, a = gamma*invstd, b = beta, so that y = (x-mean)*a + b.
 * running_mean and running_var: both given, or both NULL (no update); every other pointer is required (here, in
 * mmego_bn_finalize and in the pair form).  rows == 1: the running variance takes the biased value, 0.
 * partial_ws: 3*C*mmego_colstats_nblk(rows) floats.   Replaces native_batch_norm (train) of
 * Upper_Net.py:253-255,282-284, Lower_Net.py:51-53, GCN.py:106,117,136,310. */
int mmego_colstats_nblk(long rows);
int mmego_bn_train_stats(void* stream, const float* X, long ldx, long rows, int C, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                         float* partial_ws, float* mean, float* invstd, float* a, float* b);
/* The second half of mmego_bn_train_stats alone: partial = nblk records (n, mean, M2) per channel, [C][nblk][3], produced by a
 * kernel that had the tensor in its hands anyway (mmego_graph_mix's `stats`).  nblk <= 1024. */
int mmego_bn_finalize(void* stream, const float* partial, int nblk, int C, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float* mean, float* invstd, float* a,
                      float* b);
/* The same for two tensors of one shape in the same two launches (st_gcn's BatchNorms of tcn(x) and residual(x), GCN.py:140-147;
 * the second rides along as channels [C, 2C); same results as two calls).  partial_ws: 6*C*nblk floats; C a multiple of the
 * 8..64-wide column tile. */
int mmego_bn_train_stats_pair(void* stream, long rows, int C, float* partial_ws,
                              const float* X1, long ldx1, const float* gamma1, const float* beta1, float* running_mean1,
                              float* running_var1, float momentum1, float eps1, float* mean1, float* invstd1, float* a1, float* b1,
                              const float* X2, long ldx2, const float* gamma2, const float* beta2, float* running_mean2,
                              float* running_var2, float momentum2, float eps2, float* mean2, float* invstd2, float* a2, float* b2);
/* Eval mode: the same four vectors from the running statistics. */
int mmego_bn_eval_affine(void* stream, int C, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, float* mean, float* invstd, float* a, float* b);
/* Eval mode: fold BatchNorm(running statistics) into the preceding k=1 conv / Linear: Wf = s W, bf = (b - mean) s + beta with
 * s = gamma / sqrt(var + eps); the product then applies bias + ReLU in its epilogue (Upper_Net.py:253-255 etc. in eval). */
int mmego_bn_fold_linear(void* stream, const float* W, const float* b, int N, int K, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps, float* Wf, float* bf);
/* Eval-mode pointwise MLP: Y = relu(W3 relu(W2 relu(W1 x + b1) + b2) + b3) per row, one kernel, intermediates in LDS
 * (BasePointNet / GlobalPointNet of Upper_Net.py:242-301, Lower_Net.py:40-72 in eval mode).
 * bn == NULL: W, b are BN-folded already (mmego_bn_fold_linear).  Otherwise bn is a HOST array of 12 device pointers
 * {gamma, beta, running_mean, running_var} x 3 layers and W, b are the raw conv parameters (b may be NULL): the kernel folds
 * BatchNorm(eps) into them while staging the weights, with mmego_bn_fold_linear's arithmetic (same bits).
 * Cin, C1 <= 32; C2, C3 <= 64.  X, Y may be column slices (row strides ldx, ldy).
 * pre (0..4, <= Cin): the first `pre` input columns of every row are also written in FRONT of the row's outputs, Y[row * ldy - pre + c]
 * (Lower_Net.py:229-233's cat(xyz, features) written row by row in one launch); 0: nothing outside Y's columns is written. */
int mmego_mlp3_eval(void* stream, const float* X, long ldx, long rows, int Cin, const float* W1, const float* b1, int C1,
                    const float* W2, const float* b2, int C2, const float* W3, const float* b3, int C3, float* Y, long ldy,
                    const float* const* bn, float eps, int pre);
/* The same with the three stages' operands (folded weights, stage inputs) rounded to bf16 and fp32 accumulation (mlp3_bf16.hip; opt-in
 * precision mode of eval forwards).  Biases, ReLU and Y stay fp32. */
int mmego_mlp3_eval_bf16(void* stream, const float* X, long ldx, long rows, int Cin, const float* W1, const float* b1, int C1,
                         const float* W2, const float* b2, int C2, const float* W3, const float* b3, int C3, float* Y, long ldy,
                         const float* const* bn, float eps, int pre);
/* Y = act((X1-m1)*a1+b1 [+ (X2-m2)*a2+b2]) -- BN apply + ReLU, and the st_gcn "tcn(x)+residual" join
 * (GCN.py:140-147). */
int mmego_affine_act(void* stream, const float* X1, long ld1, const float* m1, const float* a1, const float* b1,
                     const float* X2, long ld2, const float* m2, const float* a2, const float* b2, float* Y, long ldy,
                     long rows, int C, int relu);
/* Y[:, :C] (+)= X[:, :C] with row strides: the torch.cat pieces of Upper_Net.py:266, Lower_Net.py:70,111,119. */
int mmego_copy2d(void* stream, const float* X, long ldx, float* Y, long ldy, long rows, int C, int accumulate);
/* Y[i,:] = X[idx[i],:] (rows of W floats, idx int64; indices outside [0,nsrc) give zero rows): minibatch assembly from
 * the HBM-resident dataset -- replaces the DataLoader collate + per-batch host->device copies of Train_Upper.py:140-150. */
int mmego_gather_rows(void* stream, const float* X, long nsrc, long W, const long long* idx, long nout, float* Y);
/* Point clouds packed on the device, a fresh random packing per output frame (frame_pack.hip; data.FrameStore under --point_keep).
 * pts [P][5] holds every frame's raw returns (x, y, z, intensity, velocity), frame f owning rows frame_off[f] .. frame_off[f+1]
 * (int64 CSR offsets); output frame q = 0 .. nout-1 packs frame f = frame_idx[q] into out[q] [pc_no][6] as data.pack_points does:
 *   convert  (x, y, z, intensity, velocity) -> (x, y, z, r, velocity, intensity), r = sqrtf(x*x + y*y + z*z) in fp32;
 *   keep     n = min(frame_off[f+1] - frame_off[f], max_n) points (n <= 0: an all-zero frame); point j < n survives when
 *            (key(KK, q, j) >> 8) * 2^-24 < keep_p (fp32; keep_p = 1 keeps all); if none survives, the point with the smallest
 *            (key(KO, q, j), j) does.  The survivors in increasing j are Q[0 .. n');
 *   place    n' <  pc_no: slot s receives Q[rank(s)], rank over the slots by (key(KO, q, s), s), if rank(s) < n', else six zeros;
 *            n' >= pc_no: slot r receives the survivor of rank r, rank over the survivors by (key(KO, q, j), j), j the point's number.
 * The integer recipe (32-bit unsigned arithmetic; hash32 and dropout_key as in csrc/common.h):
 *   KK = dropout_key(seed, 0x4b454550), KO = dropout_key(seed, 0x4f524452)        -- the keep and the ordering stream of a launch
 *   key(K, q, i) = hash32(hash32(K ^ hash32((unsigned)q)) ^ (unsigned)i)
 * q, not f, is the counter: a frame listed twice in one launch (overlapping windows) gets two independent packings.  The same seed
 * gives the same output, bit for bit.  Refused: null pointers, nout < 1 or >= 2^31, pc_no outside [1, 1024], max_n < 1 or beyond what
 * 64 KB of LDS hold (4 waves x (max(max_n, pc_no) + max_n) words), keep_p outside (0, 1], out not 8-byte aligned.  The caller answers for
 * frame_idx lying inside the offset array. */
int mmego_pack_frames(void* stream, const float* pts, const long long* frame_off, const long long* frame_idx, long nout,
                      int pc_no, int max_n, float keep_p, unsigned long long seed, float* out);
/* mmego_pack_frames with radar-return noise (data.FrameStore under --point_noise / --point_noise_v): keep, place and convert as above,
 * from the same two streams -- with the same seed and keep_p the same returns land in the same slots and the zero rows are the same
 * rows -- and every kept return is perturbed before its row is written.  Return j (its number inside its frame) of output frame q:
 *   KN      = dropout_key(seed, 0x4e4f4953)                      -- a third stream of the launch
 *   b       = key(KN, q, j)
 *   h(c, i) = hash32(b + (unsigned)(4 c + i + 1))  (mod 2^32)    -- c = 0, 1, 2: x, y, z; c = 3: velocity; i = 0 .. 3
 *   s_c     = sum_i (h(c, i) >> 10)                              -- four 22-bit integers, s_c < 2^24
 *   z_c     = (float)((int)s_c - 8388606) * C                    -- C = 0x1.bb67aep-22f (bits 0x34ddb3d7: fp32 nearest to sqrt(3) 2^-22)
 *   v'_c    = v_c + sigma_c * z_c                                -- sigma_c = sigma_xyz for c < 3, sigma_v for c = 3
 * z_c is the centred sum of four uniforms (Irwin-Hall): mean 0, variance 1 - 2^-44, support +-2 sqrt(3) (about +-3.46), so the jitter is
 * bell-shaped and clipped by construction.  The int -> float conversion is exact, the product and the sum are two separately rounded fp32
 * operations (never a fused multiply-add): tests/point_noise_ref.py restates every bit in integer and fp32 numpy arithmetic, which a
 * Box-Muller Gaussian would not allow.  A component whose sigma is 0 is copied, not computed (-0.0 + 0.0 * z would lose the sign).  r is
 * formed from the perturbed x, y, z; intensity is never touched.  The noise is a function of (seed, q, j): it depends neither on which
 * other returns were kept nor on the slot, and a frame listed twice gets two independent draws.  No LDS beyond mmego_pack_frames'.
 * Refused: what mmego_pack_frames refuses, and a sigma that is negative, NaN or infinite.  sigma_xyz = sigma_v = 0: mmego_pack_frames'
 * output, bit for bit. */
int mmego_pack_frames_noise(void* stream, const float* pts, const long long* frame_off, const long long* frame_idx, long nout,
                            int pc_no, int max_n, float keep_p, unsigned long long seed, float sigma_xyz, float sigma_v, float* out);
/* Head-pose noise (pose_noise.hip; train_step.StageStep under pose_noise_deg / pose_noise_t, processors._epoch_eval and dense.dense_infer under
 * pose_noise): row i = 0 .. n-1 of the head poses R [n][3][3] (row-major) and t [n][3] perturbed into R_out, t_out.  seed_word is ONE
 * int64 word ON THE DEVICE, read by the kernel: a launch captured into a HIP graph sees the word the host wrote before the replay (the
 * convention of mmego_seed_take / mmego_lstm_dropout).  ids (int64 on the device, may be NULL) gives every row its draw number
 * d = ids[i], else d = i: rows with one draw number get one draw.  With hash32 and dropout_key as in csrc/common.h:
 *   K       = dropout_key((unsigned long long)seed_word[0], 0x504F5345)         -- the launch's stream
 *   b       = hash32(K ^ hash32((unsigned)d))                                    -- the row's word
 *   z_c     = mmego_pack_frames_noise's z_c of b, c = 0 .. 5                     -- six draws of unit variance, |z_c| <= 2 sqrt(3)
 *   w       = (sigma_deg pi / 180) (z_0, z_1, z_2) in double, theta = |w|
 *   E       = I + a [w]x + b' [w]x^2,  a = sin(theta) / theta,  b' = (1 - cos(theta)) / theta^2;  for theta < 1e-3 the series
 *             a = 1 - theta^2/6 + theta^4/120,  b' = 1/2 - theta^2/24 + theta^4/720
 *   R_out   = (float)(E R): products and sums in double, one float store per entry
 *   t_out_c = (float)((double)t_c + sigma_t z_{3+c})
 * E multiplies from the left: a rotation on the head-frame side of R (xyz - t); w being isotropic, composing on the other side has the
 * same distribution.  sigma_deg is the standard deviation of the rotation vector PER AXIS, in degrees: the RMS rotation angle is
 * sqrt(3) sigma_deg and no row turns by more than 6 sigma_deg; sigma_t is in t's units and no component moves by more than 3.47 sigma_t.
 * sigma_deg == 0 copies R bit for bit, sigma_t == 0 copies t bit for bit.  One thread per row, no LDS, no atomics; two launches with one
 * word give the same bytes.  Refused (non-zero, nothing launched): a null R, t, R_out, t_out or seed_word; n < 1 (or >= 2^40); a sigma
 * that is negative, NaN or infinite; both sigmas 0; a seed_word or ids that is not 8-byte aligned; an output that overlaps an input other
 * than R_out == R or t_out == t exactly (a thread reads its row before it writes it); R_out overlapping t_out. */
int mmego_pose_jitter(void* stream, const float* R, const float* t, long n, double sigma_deg, double sigma_t,
                      const long long* seed_word, const long long* ids, float* R_out, float* t_out);
/* IMU sensor noise and bias (imu_noise.hip; train_step.ImuStep / StageStep under imu_noise, processors._epoch_eval and dense.dense_infer under
 * imu_noise): the IMU samples imu [n_rows][S][15] that IMU_Net reads perturbed into out.  A row is one frame, n_rows = B T rows in B
 * windows of T (row i belongs to window i / T), a frame has S samples, a sample is 15 floats: the orientation O [3][3] row-major
 * (channels 0 .. 8), the accelerometer (9 .. 11), the gyroscope (12 .. 14).  Every sample gets WHITE noise of its own and the BIAS of its
 * window: an offset that is constant over the window's T S samples.  seed_word is ONE int64 word ON THE DEVICE, read by the kernel
 * (mmego_pose_jitter's convention: a captured launch draws afresh once the host rewrites the word).  row_ids [n_rows] and win_ids
 * [n_rows / T] (int64 on the device, either may be NULL) give the draw numbers d = row_ids[i], else i, and u = win_ids[i / T], else i / T.
 * With hash32 and dropout_key as in csrc/common.h, for sample s = 0 .. S-1 of row i:
 *   K_s = dropout_key((unsigned long long)seed_word[0], 0x494D554E),  K_w = dropout_key((unsigned long long)seed_word[0], 0x494D5542)
 *   e   = (unsigned)(d S + s),  b_s = hash32(K_s ^ hash32(e))        -- the sample's word
 *   b_w = hash32(K_w ^ hash32((unsigned)u))                          -- the window's word: every sample of every row of a window
 *   z_s[c], z_w[c] = mmego_pack_frames_noise's z_c of b_s, b_w, c = 0 .. 8: rotation 0 .. 2, accelerometer 3 .. 5, gyroscope 6 .. 8
 *   E_s = mmego_pose_jitter's E of (noise_rot_deg pi / 180) z_s[0..2],  E_w = the same of (bias_rot_deg pi / 180) z_w[0..2]
 *   E   = E_s E_w: a 3 x 3 double product, every entry a three-term sum in column order; a factor whose sigma is 0 is left out exactly
 *   O'  = (float)(E O), as mmego_pose_jitter's R_out (from the left, as there)
 *   a'_k = (float)(((double)a_k + bias_acc z_w[3+k]) + noise_acc z_s[3+k]);  g'_k the same with bias_gyro, noise_gyro and channels 6+k
 * Everything in double, one float rounding per output.  A group (orientation, accelerometer, gyroscope) both of whose sigmas are 0 is
 * copied bit for bit.  Angles are degrees PER AXIS of the rotation vector, additive sigmas are in the recordings' units.  Bounds: no
 * additive channel moves by more than 3.47 (bias + noise); neither rotation factor turns by more than 6 times its sigma.  One launch, one
 * thread per sample (2048 workgroups of 256 at the most, strided beyond), no LDS, no atomics; out may be imu exactly (a thread reads its
 * sample before it writes it); the output is a function of the input, the word and the ids: two launches under one word write the same
 * bytes.  Refused (non-zero, nothing launched): a null imu, out or seed_word; n_rows < 1, T < 1, S < 1, n_rows % T != 0 (or n_rows S >=
 * 2^40); a sigma that is negative, NaN or infinite; all six sigmas 0; a seed_word, row_ids or win_ids that is not 8-byte aligned; out
 * overlapping imu other than out == imu exactly. */
int mmego_imu_jitter(void* stream, const float* imu, long n_rows, int T, int S,
                     double noise_rot_deg, double noise_acc, double noise_gyro,
                     double bias_rot_deg, double bias_acc, double bias_gyro,
                     const long long* seed_word, const long long* row_ids, const long long* win_ids,
                     float* out);
/* Dense inference (blend.hip; dense.dense_infer): every frame's row blended from the rows of the overlapping windows that cover it.
 * src [nrows][C] contiguous; the cover of frame f = 0 .. F-1 is the CSR list k in [cov_off[f], cov_off[f+1]) (int64 offsets) of source
 * rows cov_row[k] (int32) with weights cov_w[k]:
 *   dst[f, c] = (sum_k w_k src[row_k, c]) / (sum_k w_k), c < C; the columns of dst[f] (row stride ldd) beyond C are not touched;
 *   spread[f] (spread may be NULL; needs C % 3 == 0, J = C / 3) = sqrt(sum_k w_k sum_j |x_kj - m_j|^2 / (J sum_k w_k)), x_kj the j-th
 *               3-vector of row_k and m the blend as a double, before its rounding: the weighted RMS distance of the windows' joints
 *               from the blended joint -- how much the windows disagree about the frame.
 * Products and sums in double in CSR order, the J joints' sum in a fixed tree, one float store: a frame covered once receives its row
 * bit for bit ((w x) / w is exact in double for fp32 w, x), and two launches give the same bits.  An empty list, or weights that sum to
 * zero, give a zero row and spread 0; no NaN is made here.  One wave per frame, one lane per column: C <= 64.  Refused: a null src,
 * cov_off, cov_row, cov_w or dst, F < 1 or >= 2^31, C outside [1, 64], ldd < C, spread with C % 3 != 0.  The caller answers for cov_off
 * ascending from 0 and for cov_row lying in [0, nrows) (ops.blend_windows checks both on the host); an entry outside is skipped. */
int mmego_blend_windows(void* stream, const float* src, long nrows, int C, const long long* cov_off, const int* cov_row,
                        const float* cov_w, long F, float* dst, long ldd, float* spread);
/* out[p, c] = sum over the rows r = p (mod period) of X[r, c], p < period, c < C <= 64: a per-row table of windows of `period` frames
 * folded by position in the window ([W*T][43] joint errors -> [T][43]).  rows % period == 0, 1 <= period <= 64, ldx >= C, ldo >= C.
 * One workgroup per phase: its rows are dealt round-robin to 16 waves, each sums its share in ascending order in double, the 16
 * partial sums are added in wave order, one float store (two launches give the same bits; no workspace, no atomics). */
int mmego_colsum_phase(void* stream, const float* X, long ldx, long rows, int C, int period, float* out, long ldo);
/* The error breakdown of the evaluation passes (breakdown.hip; evaluation.breakdown_launches): a per-row table reduced by a group id
 * per row.  X [rows][C] (row stride ldx >= C), 1 <= C <= 64, 1 <= rows < 2^24; group [rows] int32; 1 <= G <= 65535:
 *   out[g, c] = the sum of X[r, c] over the rows r with group[r] == g, g < G, c < C; the columns of out[g] (row stride ldo >= C) beyond
 *               C are not touched;   count[g] (count may be NULL) = the number of those rows, as a float (exact: rows < 2^24).
 * A row whose id lies outside [0, G) belongs to no group: its values are never read into a sum (selected out, not multiplied by zero),
 * so a NaN or an Inf there reaches no output.  A group without rows gets zeros and count 0.  The rows need not be sorted by group.
 * One workgroup per group; the table is cut into blocks of 64 rows, dealt round-robin to the 16 waves of the workgroup; a wave adds the
 * group's rows of its blocks in ascending row order in double, one lane per column; the 16 partial sums are added in wave order, one
 * float store.  The order depends on (rows, G) and on which rows the group owns, on nothing else: two launches give the same bits.  No
 * workspace, no atomics, out needs no zeroing.  Refused (non-zero, nothing launched): a null X, group or out; rows < 1 or >= 2^24; C
 * outside [1, 64]; G outside [1, 65535]; ldx < C; ldo < C. */
int mmego_colsum_groups(void* stream, const float* X, long ldx, long rows, int C, const int* group, int G, float* out, long ldo,
                        float* count);
/* Integer histograms of the non-negative values of the same kind of table, by the same kind of group id (group NULL: one group of all
 * rows, G = 1).  The bin of a value x, with the product in fp32 and the comparisons in this order:
 *   x is NaN or x < 0:                      not binned; counted in dropped
 *   x * inv_width >= nbins - 1 (+Inf too):  the last bin, nbins - 1, the overflow bin (decided before any float-to-int conversion)
 *   otherwise:                              bin (int)(x * inv_width)
 * pool = 1: the C columns of a group's rows go into one histogram, hist [G][nbins] and dropped [G] (both int32);
 * pool = 0: one histogram per group and column, hist [G][C][nbins] and dropped [G][C].
 * Rows whose id lies outside [0, G) are ignored.  Counts are exact.  One workgroup per histogram: LDS integer counters (integer adds
 * commute, so the LDS atomics keep two launches bit-equal), then plain stores of the finished histogram -- every word of hist and
 * dropped is written, neither needs zeroing; no global atomics, no workspace.  Refused: a null X, hist or dropped; a null group with
 * G != 1; rows < 1 or >= 2^24; C outside [1, 64]; G outside [1, 65535]; ldx < C; nbins outside [1, 4096]; pool other than 0 or 1;
 * inv_width that is not finite and > 0. */
int mmego_hist_groups(void* stream, const float* X, long ldx, long rows, int C, const int* group, int G, float inv_width, int nbins,
                      int pool, int* hist, int* dropped);
/* The same blend with every bone's length kept (blend_bones.hip; dense.dense_infer under blend_space="bones").  src [nrows][3 J]
 * holds rigid skeletons of J joints (3-vectors x_j) and the cover is mmego_blend_windows'; bones [NB][2] (int32, on the device) lists
 * (child, parent) joint numbers in walk order -- every joint a child at most once, every parent a root (a joint that is no bone's child)
 * or an earlier bone's child -- and bone_len [NB] (float, on the device) the lengths L_b.  Per frame, with its valid entries k (those
 * whose row lies in [0, nrows)) in CSR order, their weights w_k and W = sum_k w_k:
 *   no valid entry, or W == 0: a zero row, spread 0, fallback 0;   exactly one valid entry: its row, bit for bit;   otherwise
 *   a root r:            pos_r = (sum_k w_k x_kr) / W, mmego_blend_windows' own arithmetic: those columns carry the same bits;
 *   bone b = (c, p):     s = sum_k w_k (x_kc - x_kp), every difference formed in double;
 *                        u = s / |s| where |s| > 1e-9 W L_b (and > 0), else -- the FALLBACK, counted in fallback[f] -- the normalised
 *                        difference x_kc - x_kp of the entry with the largest weight (the first such on ties), or the zero vector where
 *                        that difference is zero too;   pos_c = pos_p + L_b u, the bones taken in their listed order;
 *   dst[f, 3 j + i] = (float) pos_j[i]: positions stay doubles until this one store; the columns of dst[f] beyond 3 J are not touched;
 *   spread[f] (may be NULL) = mmego_blend_windows' spread against pos, the rigid positions before their rounding;
 *   fallback[f] (int32, may be NULL) = the number of bones of the frame that took the fallback.
 * Every blended bone has length L_b up to the rounding of its two endpoints.  No atomics, sums in a fixed order: two launches give the
 * same bits.  One wave per frame, one lane per joint, the parent's position handed over by wave shuffles.  Refused: a null src, cov_off,
 * cov_row, cov_w or dst, F < 1 or >= 2^31, J outside [1, 21], NB outside [0, J - 1], null bones or bone_len with NB > 0, ldd < 3 J.  The
 * caller answers for the cover as for mmego_blend_windows and for the bone list (ops.blend_bones checks both on the host); a bone that
 * names a joint outside [0, J) is left out, its child stays a root. */
int mmego_blend_bones(void* stream, const float* src, long nrows, int J, const long long* cov_off, const int* cov_row,
                      const float* cov_w, long F, const int* bones, const float* bone_len, int NB, float* dst, long ldd,
                      float* spread, int* fallback);
/* out[r, b] = | |x_rc - x_rp| - L_b | for the rows X [n][3 J] (row stride ldx) and the bones (c, p) = bones[b] with lengths bone_len[b]
 * as above: in double, one float store, out [n][NB] (row stride ldo) -- a per-row table for mmego_colsum, as the error tables are.
 * Refused: null pointers, n < 1 or >= 2^26, J outside [1, 21], NB outside [1, J - 1], ldx < 3 J, ldo < NB. */
int mmego_bone_length_dev(void* stream, const float* X, long ldx, long n, int J, const int* bones, const float* bone_len, int NB,
                          float* out, long ldo);
/* The blend in ROTATION space (blend_rot.hip; dense.dense_infer under blend_space="rot"): every bone's world-frame rotation
 * averaged over the cover, the nets' forward kinematics run once on the averages.  src [nrows][3 J] and the cover are
 * mmego_blend_bones'; q [nrows][NQ][9] holds the rotations the net predicted for every row (row-major 3 x 3, head frame), Rh [nrows][9]
 * the head rotation every row was run with (the head-to-world transform is p <- Rh^T p + t); bones [NB][2] (int32, on the device) is
 * mmego_blend_bones' walk table, rot_idx [NB] (int32) names the one of a row's NQ rotations that turns bone b, body [NB][3] (float) the
 * rest bone vectors.  Per frame, with its valid entries k (those whose row r_k lies in [0, nrows)) in CSR order, their weights w_k and
 * W = sum_k w_k:
 *   no valid entry, or W == 0: a zero row, zero quaternions, spread 0, rot_spread 0, fallback 0;   otherwise
 *   bone b = (c, p):     A_k = Rh[r_k]^T q[r_k][rot_idx[b]], the bone's world rotation in entry k;  S = sum_k w_k A_k;
 *                        Qbar_b = the proper rotation that maximises tr(Q^T S) -- the weighted chordal mean of the A_k, Markley's
 *                        quaternion mean: its unit quaternion (w, x, y, z) is the eigenvector of the largest eigenvalue of the
 *                        symmetric 4 x 4 matrix (S 1-indexed)
 *                          [ S11+S22+S33   S32-S23       S13-S31       S21-S12     ]
 *                          [ .             S11-S22-S33   S12+S21       S13+S31     ]
 *                          [ .             .            -S11+S22-S33   S23+S32     ]
 *                          [ .             .             .            -S11-S22+S33 ]
 *                        by cyclic Jacobi sweeps (a single rotation has the eigenvalues 3 W and three times -W);
 *                        where the two largest eigenvalues lie no more than 1e-9 W apart the mean has no direction: the FALLBACK,
 *                        counted in fallback[f], is the quaternion, by the same route, of the A_k of the entry with the largest weight
 *                        (the first such on ties);   the quaternion's sign is canonical: its first non-zero component is positive;
 *   quat[f, b] = (float4) that quaternion: one 16-byte store;
 *   exactly one valid entry: dst[f] is its row of src, bit for bit, and rot_spread[f] = 0;   otherwise
 *   a root r:            pos_r = (sum_k w_k x_kr) / W, mmego_blend_windows' own arithmetic: those columns carry the same bits;
 *   bone b = (c, p):     pos_c = pos_p + Qbar_b body_b, the bones taken in their listed order;
 *   dst[f, 3 j + i] = (float) pos_j[i]: positions stay doubles until this one store; the columns of dst[f] beyond 3 J are not touched;
 *   spread[f] (may be NULL) = mmego_blend_windows' spread against pos, the rigid positions before their rounding;
 *   rot_spread[f] (may be NULL) = sqrt(sum_b sum_k w_k theta_kb^2 / (NB W)) in radians, theta_kb the angle of D = Qbar_b^T A_k taken as
 *                        atan2(|v|, (tr D - 1) / 2), v = (D32 - D23, D13 - D31, D21 - D12) / 2: how much the windows disagree about the
 *                        frame's rotations;
 *   fallback[f] (int32, may be NULL) = the number of bones of the frame that took the fallback.
 * Every blended bone has the length |body_b| up to the rounding of its two endpoints.  All arithmetic in double from the fp32 inputs, no
 * atomics, no LDS, sums in a fixed order: two launches give the same bits.  One wave per frame, one lane per joint (the bone whose child
 * it is), the parent's position handed over by wave shuffles.  Rh is NOT checked to be a proper rotation: the nets' and the loader's head
 * rotations are, and a q or Rh that is only a rotation up to fp32 rounding is projected by the mean itself.  Refused: a null src, q, Rh,
 * cov_off, cov_row, cov_w, bones, rot_idx, body, dst or quat, F < 1 or >= 2^31, nrows < 0 or >= 2^31, J outside [2, 21], NB outside
 * [1, J - 1], NQ outside [1, 64], ldd < 3 J, a quat that is not 16-byte aligned.  The caller answers for the cover and the bone list as
 * for mmego_blend_bones and for rot_idx lying in [0, NQ) (ops.blend_rot checks all three on the host); a bone that names a joint outside
 * [0, J) or a rotation outside [0, NQ) is left out: its child stays a root and its quaternion is not written. */
int mmego_blend_rot(void* stream, const float* src, long nrows, int J, const float* q, int NQ, const float* Rh,
                    const long long* cov_off, const int* cov_row, const float* cov_w, long F, const int* bones, const int* rot_idx,
                    const float* body, int NB, float* dst, long ldd, float* quat, float* spread, float* rot_spread, int* fallback);
/* Dense inference's temporal smoothing (smooth.hip; dense.dense_infer with smooth=(H, order, taper)): a zero-phase local-polynomial
 * filter along the frames.  src [F][C] (row stride lds), seg [F] (int32) the segment of every frame (-1: none), w [2 H + 1] (float,
 * positive and finite; the host makes the taper, ops.smooth_frames checks it) the weights of the taps k = -H .. H.  Per frame f:
 *   tap k is VALID when 0 <= f + k < F and seg[f + k] == seg[f] >= 0; n of them;
 *   n <= 1 (seg[f] < 0, or f alone in its segment): dst[f, :C] = src[f, :C] bit for bit, moved[f] = 0;   otherwise
 *   deg = min(D, n - 1);  S_m = sum over the valid taps of w_k k^m, m = 0 .. 2 deg, in double;
 *   A = the first row of the inverse of the moment matrix [S_{i+j}] (i, j <= deg), in closed form by cofactors;
 *   c_k = w_k (A . [1, k, k^2][:deg + 1])   -- the weights with which the weighted least-squares polynomial of degree deg through the
 *         valid taps is evaluated at k = 0; sum_k c_k = 1;
 *   dst[f, c] = (float) sum_k c_k src[f + k, c], c < C, in double over the valid taps in ascending k; the columns of dst[f] (row
 *         stride ldd) beyond C are not touched;
 *   moved[f] (may be NULL; needs C % 3 == 0, J = C / 3) = sqrt(sum_j |y_j - x_j|^2 / J), y the filtered row as doubles, before its
 *         rounding, x = src[f]: the RMS distance over the joints that the filter moved the frame.
 * No atomics, sums in a fixed order: two launches give the same bits.  One wave per frame; lane = tap for the coefficients (2 H + 1 <=
 * 63), lane = column for the sums (C <= 64).  Refused: a null src, seg, w or dst, F < 1 or >= 2^31, C outside [1, 64], lds or ldd < C, H
 * outside [1, 31], D outside [0, 2], moved with C % 3 != 0, dst rows that overlap the src rows (the filter cannot run in place). */
int mmego_smooth_frames(void* stream, const float* src, long lds, long F, int C, const int* seg, const float* w, int H, int D,
                        float* dst, long ldd, float* moved);
/* The same filter with every bone's length kept (dense.dense_infer under blend_space="bones"): src [F][3 J] holds skeletons of J
 * joints, bones [NB][2] and bone_len [NB] are mmego_blend_bones' walk table and lengths.  Per frame, with n, deg and c_k as above:
 *   n <= 1: the row bit for bit, moved 0, fallback 0;   otherwise
 *   a root r:            pos_r = sum_k c_k x_kr, mmego_smooth_frames' own arithmetic: those columns carry the same bits;
 *   bone b = (c, p):     s = sum_k c_k (x_kc - x_kp), every difference formed in double, ascending k;
 *                        u = s / |s| where |s| > 1e-9 L_b, else -- the FALLBACK, counted in fallback[f]; c_k can be negative for deg 2,
 *                        so the sum can cancel -- the normalised bone x_c - x_p of frame f itself (tap 0), or the zero vector where
 *                        that is zero too;   pos_c = pos_p + L_b u, the bones taken in their listed order;
 *   dst[f, 3 j + i] = (float) pos_j[i];   moved[f] (may be NULL) as above against pos;   fallback[f] (int32, may be NULL) = the number
 *   of bones of the frame that took the fallback.
 * Every filtered bone has length L_b up to the rounding of its two endpoints.  One wave per frame; lane = tap, then lane = joint, the
 * parent's position handed over by wave shuffles.  Refused: a null src, seg, w or dst, F < 1 or >= 2^31, J outside [1, 21], lds or ldd <
 * 3 J, H outside [1, 31], D outside [0, 2], NB outside [0, J - 1], null bones or bone_len with NB > 0, dst rows that overlap the src rows.
 * The caller answers for the bone list (ops.smooth_bones checks it on the host); a bone that names a joint outside [0, J) is left out. */
int mmego_smooth_bones(void* stream, const float* src, long lds, long F, int J, const int* seg, const float* w, int H, int D,
                       const int* bones, const float* bone_len, int NB, float* dst, long ldd, float* moved, int* fallback);
/* The same filter in ROTATION space (smooth.hip; dense.dense_infer under blend_space="rot" with rot_smooth=(H, order, taper)): every
 * bone's world rotation filtered along the frames, the forward kinematics run once on the filtered rotations.  src [F][3 J] (row stride
 * lds) holds the rigid frames mmego_blend_rot wrote, quat [F][NB][4] its unit quaternions (w, x, y, z), the world rotation of bone b of
 * frame f, 16-byte aligned; seg, w, H, D as for mmego_smooth_frames; bones [NB][2] and body [NB][3] are mmego_blend_rot's walk table and
 * rest bone vectors.  Per frame, with the valid taps, n, deg and c_k exactly as for mmego_smooth_frames (the same function, the same bits):
 *   n <= 1: dst[f, :3 J] = src[f] bit for bit, quat_out[f] = quat[f] bit for bit, moved, rot_moved and fallback 0;   otherwise
 *   a root r:            pos_r = sum_k c_k x_kr, mmego_smooth_frames' own arithmetic: those columns carry the same bits;
 *   bone b = (c, p):     A_k = the rotation matrix of (double) quat[f + k][b] (even in the quaternion: its sign does not matter);
 *                        S = sum_k c_k A_k over the valid taps, ascending k;  W = sum_k |c_k|, the same order;
 *                        Qbar_b = the proper rotation that maximises tr(Q^T S), by mmego_blend_rot's 4 x 4 eigenproblem and Jacobi
 *                        sweeps: for D = 0 the weighted chordal mean of the neighbouring frames' rotations, for D = 1, 2 the local
 *                        polynomial of the matrix entries projected onto the rotations (c_k can be negative);  where the two largest
 *                        eigenvalues lie no more than 1e-9 W apart -- the FALLBACK, counted in fallback[f] -- the quaternion, by the
 *                        same route, of A_0, the frame's own rotation;  canonical sign: the first non-zero component is positive;
 *                        an input that is unit only up to fp32 rounding is projected by the mean itself;
 *                        pos_c = pos_p + Qbar_b body_b, the bones taken in their listed order;
 *   dst[f, 3 j + i] = (float) pos_j[i] in one store; the columns of dst[f] (row stride ldd) beyond 3 J are not touched;
 *   quat_out[f, b] = (float4) the quaternion of Qbar_b: one 16-byte store;
 *   moved[f] (may be NULL) as mmego_smooth_frames', of pos before its rounding against src[f];
 *   rot_moved[f] (may be NULL) = sqrt(sum_b theta_b^2 / NB) in radians, theta_b the angle of Qbar_b^T A_0 taken as mmego_blend_rot's
 *                        rot_spread takes it: how far the filter turned the frame's bones;
 *   fallback[f] (int32, may be NULL) = the number of bones of the frame that took the fallback.
 * Every filtered bone has the length |body_b| up to the rounding of its two endpoints, and quat_out laid over body from dst's roots gives
 * dst.  All arithmetic in double from the fp32 inputs, no atomics, no LDS, sums in a fixed order: two launches give the same bits.  One
 * wave per frame; lane = tap for the coefficients, then lane = joint (the bone whose child it is): one 16-byte load per bone and tap,
 * nine accumulators and one Jacobi solve per lane, the parent's position handed over by wave shuffles.  Refused: a null src, quat, seg,
 * w, bones, body, dst or quat_out, F < 1 or >= 2^31, J outside [2, 21], NB outside [1, J - 1], lds or ldd < 3 J, H outside [1, 31], D
 * outside [0, 2], a quat or quat_out that is not 16-byte aligned, dst rows that overlap the src rows, quat_out overlapping quat.  The
 * caller answers for the bone list (ops.smooth_rot checks it on the host); a bone that names a joint outside [0, J) is left out: its
 * child stays a root and its quaternion is not written. */
int mmego_smooth_rot(void* stream, const float* src, long lds, long F, int J, const float* quat, int NB, const int* seg, const float* w,
                     int H, int D, const int* bones, const float* body, float* dst, long ldd, float* quat_out, float* moved,
                     float* rot_moved, int* fallback);
/* Dense inference's CAUSAL filter along time (one_euro.hip; dense.dense_infer with one_euro=(fc, beta, dc)): the one-euro filter (Casiez
 * et al. 2012), an exponential low-pass whose cutoff rises with the joint's own filtered speed.  It never reads a frame ahead of the one
 * it writes.  Units are per frame: fc (finite, > 0) the minimum cutoff in cycles per frame, beta (finite, >= 0) how much a joint's speed
 * in metres per frame raises the cutoff, in 1/metre, dc (finite, > 0) the cutoff of the speed estimate in cycles per frame.
 * src [F][3 J] (row stride lds) holds rows of J 3-vectors.  The host cuts [0, F) into R RUNS: run_off [R + 1] (int64) ascends from 0 to F,
 * run r owns the frames [run_off[r], run_off[r + 1]); run_on [R] (int32): 0 -- the run's rows are copied to dst bit for bit, moved 0 --
 * or non-zero -- the run is filtered.  With alpha(c) = w / (w + 1), w = 2 pi c, per filtered run and joint j, x_i the joint's 3-vector
 * at the run's frame i, all arithmetic in double, the state (xhat, dhat) kept in double across the frames and never re-read from dst:
 *   i = 0:   xhat_0 = x_0 (the row is copied bit for bit), dhat_0 = 0, moved 0;
 *   i >= 1:  d = x_i - xhat_{i-1};   dhat_i = dhat_{i-1} + alpha(dc) (d - dhat_{i-1});   s = |dhat_i|, the Euclidean norm of the three
 *            components;   a = alpha(fc + beta s);   xhat_i = xhat_{i-1} + a d;
 *   dst[f, 3 j + t] = (float) xhat_i[t], one store per word; the columns of dst[f] (row stride ldd) beyond 3 J are not touched;
 *   moved[f] (may be NULL) = sqrt(sum_j |xhat_ij - x_ij|^2 / J), before the rounding: mmego_smooth_frames' definition.
 * One cutoff per joint and frame, from the joint's speed: the result does not depend on the axes of the (moving) frame the joints live
 * in, and a constant run comes back bit for bit (d = 0 leaves both states as they are).  Every multiply-add above is one fma.
 * One wave per run, lane = joint; sequential along the run, the rows loaded 8 frames ahead of their use; no LDS, no atomics, a fixed
 * order: two launches give the same bits.  Refused: a null src, run_off, run_on or dst, F < 1 or >= 2^31, J outside [1, 21], lds or ldd <
 * 3 J, R outside [1, F], fc, beta or dc not finite or out of range, dst rows that overlap the src rows.  The caller answers for the runs
 * partitioning [0, F) (ops.one_euro checks them on the host); the kernel clips a run to [0, F). */
int mmego_one_euro(void* stream, const float* src, long lds, long F, int J, const long long* run_off, const int* run_on, int R, double fc,
                   double beta, double dc, float* dst, long ldd, float* moved);
/* The same filter with every bone's length kept (dense.dense_infer under blend_space="bones"): bones [NB][2] and bone_len [NB] are
 * mmego_blend_bones' walk table and lengths.  A copy run, and a filtered run's first frame: the row bit for bit, moved 0, fallback 0.
 * Per filtered run and frame i >= 1:
 *   a root r:        the recursion above on its position: the same function, the same bits as mmego_one_euro gives that joint;
 *   bone b = (c, p): the same recursion on v_i = x_ic - x_ip (the difference formed in double) with the state vhat (vhat_0 = v_0),
 *                    dhat, the speed |dhat| of the vector; the state keeps the UNNORMALISED vhat;
 *                    u = vhat_i / |vhat_i| where |vhat_i| > 1e-9 L_b, else -- the FALLBACK, counted in fallback[f] -- v_i / |v_i|, the
 *                    frame's own direction, or the zero vector where that is zero too (the bone stays on its parent);
 *                    pos_c = pos_p + L_b u, the bones taken in their listed order;
 *   dst[f, 3 j + t] = (float) pos_j[t];   moved[f] (may be NULL) as above against pos;   fallback[f] (int32, may be NULL) = the number
 *   of bones of the frame that took the fallback.
 * Every filtered bone has length L_b up to the rounding of its two endpoints.  One wave per run, lane = joint, the parent's position
 * handed over by wave shuffles.  Refused: as mmego_one_euro, and NB outside [0, J - 1], null bones or bone_len with NB > 0.  The caller
 * answers for the bone list (ops.one_euro_bones checks it on the host); a bone that names a joint outside [0, J) is left out. */
int mmego_one_euro_bones(void* stream, const float* src, long lds, long F, int J, const long long* run_off, const int* run_on, int R,
                         double fc, double beta, double dc, const int* bones, const float* bone_len, int NB, float* dst, long ldd,
                         float* moved, int* fallback);
/* Dense inference's floor (floor.hip; dense.dense_infer with floor=(mode, contact_cm, margin_cm)).  Both kernels read rows of the 8
 * lower joints, [rows][24]: local joints 0..3 are the global joints 12..15, local 4..7 the global 16..19, so the legs are (hip, knee,
 * ankle, foot) = (0, 1, 2, 3) and (4, 5, 6, 7) and the feet local 3 and 7.  ground [rows][4] is every row's plane (a, b, c, d) in the
 * frame of the row's own joints; with n = (a, b, c), nh = n / |n| and dh = d / |n| the height of a point is h(x) = nh . x + dh, in double.
 * seg [rows] (int32): < 0 marks a row that takes no part.
 * mmego_floor_stats: lo [rows][24] (row stride ldl) the predicted lower joints, tgt [rows][63] (row stride ldt) the 21-joint target,
 * contact [rows][2] the recorded contact flags as floats, H > 0 the contact height in metres; out [rows][22] (packed), 11 columns per
 * foot k, foot 0 first -- foot 0 is local joint 3, target joint 15 and contact[, 0]; foot 1 local 7, target joint 19 and contact[, 1].
 * With hp = h(predicted foot), ht = h(target foot), c the flag, every comparison strict:
 *   0 |hp - ht|   1 max(0, -hp)   2 [hp < 0]   3 [hp < H]   4 [hp < H] c   5 c   6 c max(0, hp)
 *   7 max(0, -ht)   8 [ht < 0]   9 [ht < H]   10 [ht < H] c
 * A row with seg < 0, or whose |n| is not > 1e-6, writes 22 zeros: the column sums (mmego_colsum) are sums over the rows that count.
 * Refused: a null pointer, rows < 1 or >= 2^31, ldl < 24, ldt < 63, H not finite or not > 0.
 * mmego_floor_clamp: dst[r, :24] (row stride ldd; the columns beyond stay) = src[r, :24] (row stride lds) with every leg raised whose
 * foot or ankle lies under h = margin (metres, >= 0).  dst is src itself (then ldd == lds) or shares no byte with it.  A row with
 * seg < 0 or |n| <= 1e-6 is copied bit for bit, lifted 0; the bad plane counts a fallback for both legs.  The hips are always copied
 * bit for bit.  Per leg (Hp, K, A, T):
 *   lift = max(0, margin - h(T), margin - h(A));  lift == 0: the leg's nine floats are copied bit for bit;  otherwise
 *   A' = A + lift nh;  l1 = |K - Hp|, l2 = |A - K|, v = A' - Hp, D = |v|, u = v / D;  D <= 1e-9: the leg stays, one FALLBACK;
 *   Dc = min(max(D, |l1 - l2| + 1e-6 (l1 + l2)), (l1 + l2)(1 - 1e-6));  Dc != D: one FALLBACK -- the target is out of reach, the ankle
 *        lands at reach along u and the floor is not guaranteed there;
 *   a = (l1^2 - l2^2 + Dc^2) / (2 Dc), b = sqrt(max(0, l1^2 - a^2));
 *   w = (K - Hp) minus its component along u;  |w| < 1e-4 l1 (or 0): (T - A) the same way;  that < 1e-4 |T - A| (or 0): the coordinate
 *        axis with the smallest |u_i|, the first on ties, the same way;  wh = w / |w|;
 *   K' = Hp + a u + b wh,  A'' = Hp + Dc u,  T' = A'' + (T - A), the foot from the ankle as stored.
 *   A solve that is not finite (a leg without length) leaves the leg as it was: one FALLBACK, no lift.
 *   The three joints are stored as floats.  Where that rounding leaves h(A'') or h(T'), taken in double from the stored floats, under
 *   the margin on a leg without fallback, the solve is repeated with the lift raised by what is missing plus 2^-22 of the largest
 *   coordinate (more than the rounding of a height), at most twice: the stored feet are not under the margin, and lifted reports the
 *   lift that was applied, within 1e-6 of the recipe's.
 * |K' - Hp| = l1, |A'' - K'| = l2 and T' - A'' = T - A; without a fallback h(A'') = h(A) + lift, h(T') = h(T) + lift, both >= margin up
 * to rounding.  lifted [rows] (float, may be NULL): the larger of the two legs' lifts, 0 where neither moved; fallback [rows] (int32,
 * may be NULL): the legs that fell back, 0..2.  One thread per row, no atomics: two launches give the same bits.  Refused: a null src,
 * ground, seg or dst, rows < 1 or >= 2^31, lds or ldd < 24, a margin that is not finite or < 0, dst rows that overlap the src rows
 * without being them. */
int mmego_floor_stats(void* stream, const float* lo, long ldl, const float* tgt, long ldt, const float* ground, const float* contact,
                      const int* seg, long rows, double H, float* out);
int mmego_floor_clamp(void* stream, const float* src, long lds, const float* ground, const int* seg, long rows, double margin, float* dst,
                      long ldd, float* lifted, int* fallback);
/* Dense inference's pictures (render.hip, render_math.h; mmego_amd/render.py, dense.dense_infer with render=...): a scene builder that
 * turns every frame into a table of 2-D primitives, and a tiled rasteriser that composites such tables into 8-bit RGB images.
 * A primitive is 12 floats: ax, ay, bx, by, r, alpha, cr, cg, cb, 0, 0, 0 -- a capsule from a to b in pixel coordinates (a disc where
 * a == b) of radius r pixels, opacity alpha and colour (cr, cg, cb) in levels 0..255.
 * mmego_render_raster: prims [I][P][12] (16-byte aligned) -> out (uint8), image i a W x H viewport of 3-byte pixels at
 * out + i img_stride + y row_pitch + 3 x (bytes; whatever lies between the viewport's rows stays as it is, so two views can share one
 * frame through the pitch).  The centre of pixel (x, y) is (x + 0.5, y + 0.5).  Per pixel, all in fp32: the colour starts at the
 * background (bg_r, bg_g, bg_b); the image's primitives are composited in INDEX order,
 *   d = the distance from the pixel centre to the segment ab:  t = clamp(((p - a) . (b - a)) / |b - a|^2, 0, 1), 0 where a == b,
 *       d = |p - (a + t (b - a))|;
 *   c = clamp(r + 0.5 - d, 0, 1) alpha;   colour += c (prim_colour - colour) per channel;
 * the byte stored is (int)(min(max(colour, 0), 255) + 0.5f).  A primitive contributes nothing where any of its first nine floats is
 * not finite, where alpha <= 0 or r < 0, or where |b - a|^2 overflows fp32.  The composite is continuous in every input: the order is
 * fixed, nothing is decided by "nearest wins", there is no depth test.  One workgroup of 256 threads per (image, 32 x 32 tile): 256
 * primitives at a time are culled against the tile's pixel centres grown by r + 0.5 and, on top, by 2^-21 of the coordinates'
 * magnitudes -- conservative beyond the fp32 roundings of the distance, so a culled primitive's c is 0 on the tile and culling
 * changes no byte, the survivors are compacted in index order into an LDS list (64-bit ballot, popcount prefix per wave,
 * wave offsets through LDS), and every thread composites the list into its four horizontally adjacent pixels in registers and stores
 * 12 bytes as three dwords; edge tiles mask their pixels.  No atomics, every byte has one owner: two launches give the same bytes.
 * Refused: a null pointer, I < 1, I x tiles >= 2^31, P outside [0, 1024] (0 paints the background), W or H outside [16, 2048],
 * W % 4 != 0, row_pitch < 3 W or % 4 != 0, img_stride < H row_pitch or % 4 != 0, an out that is not 4-byte aligned, prims that are
 * not 16-byte aligned, a bg level outside [0, 255].  The caller answers for out's extent (ops.render_raster checks it on the host).
 * mmego_render_prims: the scene of F frames, everything in the frame of the frame's own joints: pred [F][63] (row stride ldp) and tgt
 * [F][63] (row stride ldt) the predicted and the recorded 21 joints, ground [F][4] the floor planes (height h(x), unit normal u and
 * the rule |n| > 1e-6 as for mmego_floor_stats above), cloud [F][N][6] the radar returns (x, y, z, r, v, intensity), seg [F] int32
 * (< 0: the frame has no prediction), cam [F][8] a 2 x 4 affine per frame, x_px = m0 p_x + m1 p_y + m2 p_z + m3 and y_px the same with
 * m4..m7, ring [32][2] the pairs (cos, sin)(2 pi k / 32) as the host rounded them.  -> prims [F][P][12] with P = 134 + N, in this
 * order (the layer order; bones are skeleton.BONES_ALL's 20 (parent, child) pairs):
 *   first  count  what                                                                radius  colour        alpha
 *   0      32     floor ring: segment k joins vertex k to vertex (k + 1) % 32 of      0.5     170,170,170   1
 *                 foot + cos_k e1 + sin_k e2, foot = t0 - h(t0) u (t0 = target joint 0), e1 = the coordinate axis with the smallest
 *                 |u_i| (the first on ties) minus its component along u, normalised, e2 = u x e1: a circle of 1 m in the plane
 *   32     20     shadow: every predicted bone, both ends dropped x - h(x) u          2       60,60,60      0.35
 *   52     20     target bones                                                        1.5     120,120,120   1
 *   72     21     target joints (discs)                                               2.5     90,90,90      1
 *   93     N      cloud returns (discs), (40,90,220) + s ((230,60,40) - (40,90,220)),  1.5     by Doppler    0.8
 *                 s = clamp(0.5 + v / (2 vmax), 0, 1)
 *   93+N   20     predicted bones, (0,170,0) + s ((230,0,0) - (0,170,0)),              2       by error      1
 *                 s = min(e / 0.15, 1), e = |child - its target| in metres
 *   113+N  21     predicted joints (discs), coloured the same way by their own error  3       by error      1
 * An ABSENT primitive is twelve zeros (alpha 0: the rasteriser skips it): the ring and the shadow where the plane has no normal; the
 * shadow, the predicted bones and joints where seg < 0 (such a frame shows the target alone); a cloud row whose x, y and z are all
 * exactly 0 (padding).  Double inside, one float store per value; one thread per (frame, primitive), no LDS, no atomics.  Refused: a
 * null pointer (cloud may be NULL where N == 0), F < 1 or >= 2^31, N outside [0, 890] (so P <= 1024), ldp or ldt < 63, a vmax that is
 * not finite or not > 0, prims that are not 16-byte aligned. */
int mmego_render_raster(void* stream, const float* prims, int I, int P, unsigned char* out, int W, int H, long row_pitch, long img_stride,
                        int bg_r, int bg_g, int bg_b);
int mmego_render_prims(void* stream, const float* pred, long ldp, const float* tgt, long ldt, const float* ground, const float* cloud,
                       int N, const int* seg, const float* cam, const float* ring, long F, double vmax, float* prims);
/* BatchNorm (train) backward through an optional ReLU mask (Ymask > 0): dgamma, dbeta, dX.
 * partial_ws: 2*C*nblk floats, c12_ws: 2*C floats. */
int mmego_bn_backward(void* stream, const float* dY, long lddy, const float* Ymask, long ldm, const float* X, long ldx,
                      const float* mean, const float* invstd, const float* a, long rows, int C, float* partial_ws,
                      float* c12_ws, float* dgamma, float* dbeta, float* dX, long lddx);
/* Two BatchNorms that share dY and the mask -- st_gcn's relu(BN(tcn(x)) + BN(residual(x))), GCN.py:140-147 -- in the same three
 * launches (the second one rides along as channels [C, 2C); results are those of two mmego_bn_backward calls, bit for bit).
 * partial_ws: 4*C*nblk floats, c12_ws: 4*C floats; C a multiple of the 8..64-wide column tile (8, 16, 32, 64, 128, ...). */
int mmego_bn_backward_pair(void* stream, const float* dY, long lddy, const float* Ymask, long ldm, long rows, int C,
                           float* partial_ws, float* c12_ws,
                           const float* X1, long ldx1, const float* mean1, const float* invstd1, const float* a1,
                           float* dgamma1, float* dbeta1, float* dX1, long lddx1,
                           const float* X2, long ldx2, const float* mean2, const float* invstd2, const float* a2,
                           float* dgamma2, float* dbeta2, float* dX2, long lddx2);
/* out[c] (+)= sum_r X[r,c]: bias gradients; out2 (may be NULL) receives a copy (nn.LSTM's bias_ih / bias_hh share
 * one gradient).  partial_ws: C*nblk floats.  scale (may be NULL; rows <= 1024): the sum is multiplied by scale[c] first (the
 * edge-importance gradient = A . sum of the per-workgroup partials of mmego_graph_dA, GCN.py:62). */
int mmego_colsum(void* stream, const float* X, long ldx, long rows, int C, float* partial_ws, float* out, float* out2,
                 int accumulate, const float* scale);
/* The same for X [rows <= 1024, 2C] in ONE launch: columns [0, C) -> outA (and outA2), columns [C, 2C) -> outB (and outB2): the
 * four bias gradients of a BiLSTM layer (both directions x bias_ih / bias_hh) from its gate gradients.  C % 16 == 0. */
int mmego_colsum_pair(void* stream, const float* X, long ldx, long rows, int C, float* outA, float* outA2, float* outB,
                      float* outB2, int accumulate);
/* G = 0 where H <= 0 (ReLU backward for Linear+ReLU pairs, Upper_Net.py:350-351). */
int mmego_relu_mask(void* stream, float* G, long ldg, const float* H, long ldh, long rows, int C);
int mmego_fill(void* stream, float* X, long n, float v);

/* ---- LSTM (lstm.hip) ------------------------------------------------------------------------------
 * One timestep of a (bi)LSTM, any H % 32 == 0: gates = xproj + hprev . W_hh^T, fused cell update, c in
 * place.  Replaces the recurrent half of nn.LSTM for IMU_Net (Net/IMU_Net.py:58-62,77,82); xproj is the
 * input projection (incl. b_ih) produced by mmego_gemm, b_hh is added here.  first != 0: h_{t-1} = c_{t-1} = 0
 * (hprev may be NULL, the product is skipped).  Row strides: hps, xs, hos.  gst_d [Bn][4H] / cst_d [Bn][H]: optional
 * stash of this step's gate activations and cell state for mmego_lstm_cell_backward (training). */
int mmego_lstm_step(void* stream, int ndir, int Bn, int H, int first, const float* hprev0, const float* hprev1,
                    long hps, const float* whh0, const float* whh1, const float* bhh0, const float* bhh1,
                    const float* xproj0, const float* xproj1, long xs, float* hout0, float* hout1, long hos, float* c0,
                    float* c1, float* gst0, float* gst1, float* cst0, float* cst1);
/* Whole-sequence H=64 bidirectional LSTM layer (Upper_Net.py:333, Lower_Net.py:91, Upper_Net.py:210).
 * xproj_d rows are (b*T+t) with row stride xs; out rows (b*T+t) with row stride os, direction d in
 * columns [64d, 64d+64).  Optional stashes for backward (all or none): gates_d [T][B][64][4] (the four gate activations
 * i, f, g, o of a hidden unit side by side: a private format between this call and mmego_lstm64_backward, 16-byte aligned -- checked
 * by both calls and their _multi forms: the stash is stored and loaded 16 bytes at a time),
 * cst_d [T][B][64], hprev_d [(b*T+t)][64].
 * drop_y / drop_mask (both or neither; out's layout): nn.LSTM(dropout=drop_p)'s inverted inter-layer dropout applied while the
 * outputs are stored -- drop_mask = 0 or 1/(1-p) per element from a counter-based hash of (element index, seed_ctr[0], salt),
 * drop_y = out * drop_mask.  seed_ctr is only read; mmego_inc_i64 advances it once per training forward, salt tells the
 * call sites of one forward apart. */
int mmego_lstm64_forward(void* stream, int B, int T, const float* xproj0, const float* xproj1, long xs,
                         const float* whh0, const float* whh1, const float* bhh0, const float* bhh1, const float* h0_0,
                         const float* h0_1, const float* c0_0, const float* c0_1, float* out, long os, float* hn0,
                         float* hn1, float* cn0, float* cn1,
                         float* gates0, float* gates1, float* cst0, float* cst1, float* hprev0, float* hprev1,
                         float* drop_y, float* drop_mask, float drop_p, const unsigned long long* seed_ctr, int salt);
/* Backward through time of the same layer: dgates_d rows (b*T+t), row stride dgs (pre-activation
 * gradients; weight/input gradients follow as mmego_gemm products). */
int mmego_lstm64_backward(void* stream, int B, int T, const float* dout, long dos, const float* gates0,
                          const float* gates1, const float* cst0, const float* cst1, const float* c0_0,
                          const float* c0_1, const float* whh0, const float* whh1, float* dgates0, float* dgates1,
                          long dgs);
/* Batch rows per workgroup (4 or 16) that the four lstm64 calls take at batch size B on the current device: 4-row workgroups
 * (v_mfma_f32_4x4x1_16B_f32) while the 16-row grid, 2 x ceil(B/16) workgroups, covers at most half of the CUs, 16-row
 * ones (v_mfma_f32_16x16x4_f32) from there on.  The two forms add the terms of every product in the same order: the same bits.
 * All launches of one B take the same form.  MMEGO_LSTM64_ROWS=4|16 in the environment forces one. */
int mmego_lstm64_rows(int B);

/* The two calls above for n <= 4 INDEPENDENT stacks' layers in ONE launch (grid z = stack; descs: n host structs whose fields are the
 * argument lists above, in order).  All stacks share B and T and the options (stashes for all or none, dropout for all or none).
 * UpperNetwlocal's global and anchor BiLSTM(64) stacks (Net/Upper_Net.py:333-339 and :208-216: same shape, no data in common) run
 * layer by layer side by side this way. */
typedef struct MmegoLstm64Fwd {
  const float* xproj[2]; long xs;
  const float* whh[2]; const float* bhh[2]; const float* h0[2]; const float* c0[2];
  float* out; long os;
  float* hn[2]; float* cn[2];
  float* gates[2]; float* cst[2]; float* hprev[2];
  int B, T;
  float* drop_y; float* drop_mask; float drop_p; const unsigned long long* seed_ctr; unsigned salt;
} MmegoLstm64Fwd;
typedef struct MmegoLstm64Bwd {
  const float* dout; long dos;
  const float* gates[2]; const float* cst[2]; const float* c0[2]; const float* whh[2];
  float* dgates[2]; long dgs;
  int B, T;
} MmegoLstm64Bwd;
int mmego_lstm64_forward_multi(void* stream, int n, const MmegoLstm64Fwd* descs);
int mmego_lstm64_backward_multi(void* stream, int n, const MmegoLstm64Bwd* descs);

/* ---- bf16-operand / fp32-accumulate forward of the frozen IMU_Net (bf16.hip; BASELINE config 5) -------------------
 * Opt-in precision mode, never the parity path.  bf16 values cross the ABI as raw bits in unsigned short.
 * Y[r, 0:cols] = bf16(X[r, 0:cols]) (round to nearest even); cols, ldx, ldy multiples of 4. */
int mmego_cvt_bf16(void* stream, const float* X, long ldx, long rows, long cols, unsigned short* Y, long ldy);
/* Same with a row permutation: rows (b*T + t) of X -> rows (t*Bp + b) of Y (Bp >= Bn, pad rows untouched): the time-major
 * operand of a BiLSTM layer's input projection. */
int mmego_cvt_bf16_tm(void* stream, const float* X, long ldx, int Bn, int T, long cols, unsigned short* Y, int Bp);
/* C[M,N] = A[M,K] . W[N,K]^T + bias[N] (relu), operands bf16, products and sums fp32.  Any of three outputs (NULL = skip):
 * C (fp32 row-major), Cb (bf16 row-major), Cf (fp32 TILE-MAJOR, M % 32 == 0 and N % 32 == 0): element (m, n) at
 *     ((m/32)*(N/32) + n/32)*1024 + ((m%32)/8)*256 + (n%32 + 32*(((m%32)/4)&1))*4 + m%4,
 * i.e. every 32x32 tile stored as the MFMA accumulator holds it (coalesced 16 B per lane for producer and consumer).
 * K % 64 == 0.  Replaces the BiLSTM input projections of Net/IMU_Net.py:58-62 in bf16 mode. */
int mmego_gemm_bf16(void* stream, const unsigned short* A, long lda, const unsigned short* W, long ldw, float* C,
                    long ldc, unsigned short* Cb, long ldcb, float* Cf, const float* bias, int M, int N, int K, int relu);
/* One (bi)LSTM timestep as mmego_lstm_step, with h_{t-1} and W_hh in bf16: gates = xproj + h_{t-1} . W_hh^T (xproj
 * already holds b_ih + b_hh), cell update in fp32, c in place.  H % 64 == 0.
 * The recurrent operands are FRAGMENT-MAJOR (the order the MFMA lanes read them, so a wave's operand load is one
 * coalesced 1-KB read): element (r, k) of an [R, H] matrix sits at
 *     (((r/32)*(H/16) + k/16)*64 + ((k/8)&1)*32 + r%32)*8 + k%8        (R padded to a multiple of 32 rows).
 * hprev_d: h_{t-1} in that layout (R = Bn); whh_d: W_hh in that layout with its rows reordered to
 * [hidden block jb][gate n][32 units] (row 128*jb + 32*n + jj = W_hh[n*H + 32*jb + jj]).
 * xpf: the layer's input projection, the tile-major Cf of mmego_gemm_bf16 with M = T*Bp rows ordered t*Bp + b
 * (Bp = Bn rounded up to 32) and N = 8H columns ordered d*4H + gate*H + j; mt0_d = t_d * Bp/32 selects direction d's
 * timestep.
 * h_t is written three times: hout (fp32, row stride hos), houtb (bf16 row-major, row stride hbs, may be NULL: the next
 * layer's projection operand) and hfrag_d (bf16 fragment-major: the next step's hprev_d; must not alias hprev_d). */
int mmego_lstm_step_bf16(void* stream, int ndir, int Bn, int H, int first, const unsigned short* hprev0,
                         const unsigned short* hprev1, const unsigned short* whh0, const unsigned short* whh1,
                         const float* xpf, long mt0_0, long mt0_1, float* hout0, float* hout1,
                         long hos, unsigned short* houtb0, unsigned short* houtb1, long hbs,
                         unsigned short* hfrag0, unsigned short* hfrag1, float* c0, float* c1);

/* Large batches: the input projection folded into the step -- gates = [x_t | h_{t-1}] . [W_ih | W_hh]^T + bias in ONE fp32
 * accumulation, no projection tensor in HBM.  Up to two input segments (layer 0: x_t, K0 = In; upper layers: the previous
 * layer's forward and backward h_t, K0 = K1 = H) plus h_{t-1} (skipped when first != 0); every operand fragment-major as in
 * mmego_lstm_step_bf16 (a*_d: [Bp x K] activations of direction d's timestep; w*_d: the matching column block of W_ih with rows
 * reordered [hidden block][gate][32 units]); bias = [2][4H] b_ih + b_hh.  K0, K1, H multiples of 64.  hout_d (fp32, may be NULL
 * for layers whose output only feeds the next layer) and hfrag_d (fragment-major bf16, always) receive h_t. */
int mmego_lstm_step_bf16_fused(void* stream, int ndir, int Bn, int H, int first, int nseg,
                               const unsigned short* a0_0, const unsigned short* a0_1, const unsigned short* w0_0,
                               const unsigned short* w0_1, int K0, const unsigned short* a1_0,
                               const unsigned short* a1_1, const unsigned short* w1_0, const unsigned short* w1_1,
                               int K1, const unsigned short* hprev0, const unsigned short* hprev1,
                               const unsigned short* whh0, const unsigned short* whh1, const float* bias,
                               float* hout0, float* hout1, long hos, unsigned short* hfrag0, unsigned short* hfrag1,
                               float* c0, float* c1);
/* Attention pooling over the T timesteps of a layer run by mmego_lstm_step_bf16_fused (IMU_Net.py:77-81: softmax over t of
 * w . h_t + b, weighted sum), read from the steps' own fragment-major bf16 h_t: hf = [T][2 directions][Bp x H] (the hfrag outputs,
 * direction 0 then 1 per timestep).  The layer's step launches then need no fp32 output (hout NULL).  vec [Bn][2H] fp32 row-major,
 * attn [Bn][T] or NULL; H in {128, 256, 512} (mmego_attn_pool_frag_bf16_ok), Bp % 32 == 0. */
int mmego_attn_pool_frag_bf16_ok(int H);
int mmego_attn_pool_frag_bf16(void* stream, const unsigned short* hf, int T, int Bp, int Bn, int H, const float* w, const float* b,
                              float* vec, float* attn);
/* rows (b*T + t) of X[., C] -> T fragment-major [Bp x C] bf16 matrices (timestep t at offset t*Bp*C): a layer-0 input of
 * mmego_lstm_step_bf16_fused.  C % 16 == 0, Bp % 32 == 0. */
int mmego_cvt_bf16_frag_tm(void* stream, const float* X, long ldx, int Bn, int T, int C, unsigned short* Y, int Bp);
/* Linear(Cin <= 16, H) (+ ReLU) straight into that layout: Y[t] = bf16(act(X[b*T + t] . W^T + bias)) for rows (b*T + t) of X[., Cin]
 * (IMU_Net's fc1, Net/IMU_Net.py:53,73, as the layer-0 operand of the fused bf16 step: the fp32 activation is never stored).
 * W [H][Cin] row-major, bias [H] or NULL; H % 16 == 0, Bp % 32 == 0; rows b >= Bn are written as zeros. */
int mmego_fc_relu_bf16_frag_tm(void* stream, const float* X, long ldx, const float* W, const float* bias, int Bn, int T, int Cin,
                               int H, unsigned short* Y, int Bp, int relu);

/* ---- IMU_Net stage-1 training pieces (imu_train.hip): reference Processor/Train/Train_IMU.py:21-34,114-149 -------
 * Pointwise LSTM cell backward of one timestep, both directions: dh = dout + dh_rec (dh_rec may be NULL), reads the
 * stashed gates / cell states, writes the pre-activation gate gradients dgates_d [Bn][4H] (row stride dgs) and updates
 * dc_d [Bn][H] in place (zero it before the last timestep).  cprev_d NULL means c_{t-1} = 0.  Only dout and dgates take a
 * row stride (dos, dgs: time slices of [Bn][T][2H] / [Bn][T][8H] buffers); gst_d has the FIXED row stride 4H of mmego_lstm_step's
 * stash, and cst_d, cprev_d, dh_rec_d, dc_d are dense [Bn][H]. */
int mmego_lstm_cell_backward(void* stream, int ndir, int Bn, int H, const float* dout0, const float* dout1, long dos,
                             const float* dhrec0, const float* dhrec1, const float* gst0, const float* gst1,
                             const float* cst0, const float* cst1, const float* cprev0, const float* cprev1, float* dc0,
                             float* dc1, float* dgates0, float* dgates1, long dgs);
/* Stage-1 loss: sum acos(clamp((tr(R Rgt^T)-1)/2, +-(1-1e-7))) * 180/3.14159265358 + 100 * sum |t - head|_2 and its
 * gradients wrt R [F,3,3] and t [F,3] (scaled by `scale`). */
int mmego_imu_loss(void* stream, const float* R, const float* t, const float* R_gt, const float* head_gt, long F,
                   float scale, float* loss, float* dR, float* dt);
/* One step of a BiLSTM layer's backward recurrence, both directions: dh_rec = dgates_s [Bn][4H] (row stride dgs) . W_hh (given
 * transposed, wT [H][4H]) with the cell backward of the next step of the backward pass applied on the product's tiles (same
 * arithmetic as mmego_lstm_cell_backward: dh = dout + dh_rec; gst / cst / cprev: that step's forward stashes, cprev NULL at the
 * sequence start; dc updated in place; dgo: that step's gate gradients, row stride dgs).  Replaces product + cell-backward
 * launches of the reference's nn.LSTM autograd (Train_IMU.py:114-149).  Bn, H multiples of 32. */
int mmego_lstm_bwd_step(void* stream, int Bn, int H, const float* dg0, const float* dg1, long dgs, const float* wT0,
                        const float* wT1, const float* dout0, const float* dout1, long dos, const float* gst0,
                        const float* gst1, const float* cst0, const float* cst1, const float* cprev0, const float* cprev1,
                        float* dc0, float* dc1, float* dgo0, float* dgo1);
/* Backward of mmego_imu_head: (dR [F,3,3], dt [F,3]) -> dy [F,9]. */
int mmego_imu_head_backward(void* stream, const float* y, const float* dR, const float* dt, long F, float* dy);

/* ---- geometry, heads, loss, selection (geom.hip) --------------------------------------------------
 * In-place xyz <- R (xyz - t) per frame (Utils.py:284-292, quirk Q1: the caller's buffer is mutated).
 * src (may be NULL): the points are read from src instead of pts (copy + transform, one launch); src_ld = 3: src holds xyz only,
 * src_ld >= C: whole rows, the channels behind xyz are copied too.  keep (may be NULL, [F*P][C]) and feats (may be NULL: the first
 * nfeat channels, row stride ldf) receive the transformed rows as well (Upper_Net.py:392-395 makes those copies right behind the
 * transform).  C <= 8 when any row copy is asked for. */
int mmego_transform2h(void* stream, float* pts, long F, int P, int C, const float* R, const float* t, const float* src,
                      long src_ld, float* keep, float* feats, long ldf, int nfeat);
/* out = R^T in + t (transpose=1, add_t=1: Utils.py:274-281) or out = R in (its backward). */
int mmego_rotate_points(void* stream, const float* in, float* out, long F, int P, const float* R, const float* t,
                        int transpose, int add_t);
/* Backward of mmego_transform2h with respect to the head pose: dR [F,3,3], dR[f][i][k] = sum_n g_i (p - t)_k and dt [F,3] =
 * -R^T sum_n g over the frame's P points.  pts (row stride ldp >= 3): the UNTRANSFORMED points -- p - t is never recovered as R^T p',
 * R need not be orthonormal.  g (row stride ldg) and g2 (may be NULL, row stride ldg2): gradients with respect to the transformed xyz
 * columns of the F*P rows; their sum is used (Upper_Net: PointNet's first layer and the xyz columns of GlobalPointNet's input).
 * accumulate != 0: added to what dR / dt hold.  One wave per frame, a fixed summation order: two runs give the same bits. */
int mmego_transform2h_backward(void* stream, const float* pts, long ldp, long F, int P, const float* R, const float* t,
                               const float* g, long ldg, const float* g2, long ldg2, int accumulate, float* dR, float* dt);
/* Backward of Lower_Net's two head-frame transforms p' = R (p - t) (Lower_Net.py:191-192,205) with respect to R, t and the predicted
 * joints, in one launch.  Points share (skipped when pts is NULL): pts [F*N] UNTRANSFORMED rows (row stride ldp), idx [F,P] the
 * forward's selection (int64, indices into the frame's N rows), g (row stride ldg) and g2 (may be NULL, row stride ldg2) gradients
 * with respect to the transformed xyz of the F*P selected rows (BasePointNet's input gradient and the xyz columns of p_vec's).
 * Joints share (skipped when joints is NULL): joints [F,V,3] as the caller gave them, gj (row stride ldgj >= 3V) and gj2 (may be NULL,
 * row stride ldgj2) gradients with respect to the transformed joints, one row of 3V columns per frame (fc0's input columns and
 * data_bn's input gradient).  dR [F,3,3], dR[f][i][k] = sum g_i (p - t)_k and dt [F,3] = -R^T sum g over both shares (both NULL: not
 * wanted); djoints [F,V,3] = R^T gj (may be NULL).  accumulate != 0: added to what dR / dt hold (the world transform's share).
 * One wave per frame, a fixed summation order (points, then joints, in index order; then the lanes): two runs give the same bits. */
int mmego_lower_inputs_backward(void* stream, const float* pts, long ldp, long F, int N, const long long* idx, int P, const float* R,
                                const float* t, const float* g, long ldg, const float* g2, long ldg2, const float* joints, int V,
                                const float* gj, long ldgj, const float* gj2, long ldgj2, int accumulate, float* dR, float* dt,
                                float* djoints);
/* which=0: y[F,87] -> q[F,14,3,3], joints[F,15,3] (Upper_Net.py:122-144,354-364);
 * which=1: y[F,42] -> q[F,6,3,3], joints[F,8,3] (Lower_Net.py:12-37,125-136).  body [B,20,3]; frame n
 * uses body row n % B (quirk Q2).  Joints are in the head frame.
 * Rw [F,3,3], tw [F,3], world [F,nslots,3] (all three or none): world = Rw^T joint + tw, the head-to-world transform that follows
 * the kinematics (Upper_Net.py:362-364, Lower_Net.py:225-227; mmego_rotate_points' arithmetic) from the same launch.
 * counters / ncount / seed_ctr (0 / NULL: none): the net's once-per-training-forward tick (mmego_inc_i64) on the same launch --
 * this kernel runs once per forward, behind every reader of the dropout seed.
 * backward: Rw given -> dj is the gradient wrt the WORLD-frame joints (the head-frame gradient Rw dj is formed first). */
int mmego_head_fk_forward(void* stream, int which, const float* y, const float* body, int B, long F, float* q,
                          float* joints, const float* Rw, const float* tw, float* world, long long* counters, int ncount,
                          unsigned long long* seed_ctr);
int mmego_head_fk_backward(void* stream, int which, const float* y, const float* body, int B, long F, const float* dj,
                           float* dy, const float* Rw);
/* mmego_head_fk_backward with the head pose's own gradients of world = Rw^T joint + tw: dj is the gradient wrt the WORLD-frame joints,
 * joints_h [F,nslots,3] the forward's head-frame joints; dtw [F,3] = sum_slots dj, dRw [F,3,3], dRw[k][i] = sum_slots joint_k dj_i
 * (slots added in index order).  dy as from mmego_head_fk_backward, bit for bit. */
int mmego_head_fk_backward_pose(void* stream, int which, const float* y, const float* body, int B, long F, const float* dj,
                                float* dy, const float* Rw, const float* joints_h, float* dRw, float* dtw);
/* mmego_head_fk_backward_pose of a SECOND gradient dj wrt the world-frame joints, accumulated onto what an earlier launch left:
 * dy[f] += that call's dy;  dRw[f] = (dRw[f] + that call's dRw[f]) + dR_add[f],  dtw likewise (fp32 adds in this order).  dRw and dtw
 * both NULL: dy only (joints_h is then not read);  dR_add / dt_add NULL: that term is skipped.  One thread per frame reads and writes
 * its own rows: fixed order, two runs give the same bits.  No two of the buffers may overlap (dy / dRw / dtw are read and written, every
 * pointer is __restrict__ in the kernel): in particular dR_add / dt_add are not dRw / dtw, and dj is not a view of dy. */
int mmego_head_fk_backward_extra(void* stream, int which, const float* y, const float* body, int B, long F, const float* dj,
                                 float* dy, const float* Rw, const float* joints_h, float* dRw, float* dtw, const float* dR_add,
                                 const float* dt_add);
/* mmego_head_fk_forward -> mmego_l1_loss (scale, loss[2], gradient = sign) -> mmego_head_fk_backward as ONE launch.  The loss is a
 * fixed-order sum: per-workgroup partial pairs in scratch (2 * ceil(F/64) + 1 doubles; the last double's storage is a ticket that must
 * be 0 before the first call and is left 0), added in index order by the workgroup that finishes last.  map [nslots]: target joint of
 * every predicted slot; dy [F, ny]: d loss / d y.  Predictions and gradients bit-identical to the three calls; the two loss figures
 * agree to fp64 rounding of a different (but fixed) summation order (Train_Upper.py:165-182, Train_Lower.py:199-224). */
int mmego_head_fk_loss(void* stream, int which, const float* y, const float* body, int B, long F, float* q, float* joints_h,
                       const float* Rw, const float* tw, float* world, long long* counters, int ncount,
                       unsigned long long* seed_ctr, const float* target, const int* map, int ntgt, double scale, float* loss,
                       float* dy, double* scratch);
/* mmego_head_fk_loss with dRw [F,3,3], dtw [F,3] (see mmego_head_fk_backward_pose) from the same launch; everything else bit for bit. */
int mmego_head_fk_loss_pose(void* stream, int which, const float* y, const float* body, int B, long F, float* q, float* joints_h,
                            const float* Rw, const float* tw, float* world, long long* counters, int ncount,
                            unsigned long long* seed_ctr, const float* target, const int* map, int ntgt, double scale, float* loss,
                            float* dy, double* scratch, float* dRw, float* dtw);
/* y[F,9] -> R[F,3,3] (eps rule of IMU_Net.py:7-18), t[F,3]. */
int mmego_imu_head(void* stream, const float* y, long F, float* R, float* t);
/* IMU_Net.fc2 (Net/IMU_Net.py:84) and mmego_imu_head in one launch: y = X [F][K] . W[9][K]^T + b (row-wise dot products, fixed
 * summation structure), then R, t as mmego_imu_head; y_out [F][9] optional.  K % 256 == 0, ldx % 4 == 0. */
int mmego_imu_fc2_head(void* stream, const float* X, long ldx, const float* W, const float* b, long F, int K, float* y_out,
                       float* R, float* t);
/* loss[0] = sum |pred - target[:, map]|, grad = scale*sign(.) (L1Loss(reduction='sum'), Train_Upper.py:53,179);
 * loss[1] = sum of the per-joint Euclidean distances (the per-minibatch accuracy log, Train_Upper.py:183-185).
 * `loss` holds TWO floats. */
int mmego_l1_loss(void* stream, const float* pred, const float* target, const int* map, int nsel, int ntgt, long F,
                  float scale, float* loss, float* grad);
/* Keep the `keep` rows with the largest column-0 key, descending, ties lowest index first; idx is int64
 * (Lower_Net.py:216-227). */
int mmego_topk_rows(void* stream, const float* pts, long F, int N, int C, int keep, float* out, long long* idx);
/* Per-frame evaluation figures of `--infer` (Processor/Test/Demo_test.py:64-69,121-123,150-163):
 * E[f,0:21] joint errors (m) of the assembled 21-joint skeleton, E[f,21:41] bone angles (deg),
 * E[f,41] mean upper-joint error, E[f,42] mean lower-joint error.  Means over frames via mmego_colsum. */
int mmego_pose_errors(void* stream, const float* upper, const float* lower, const float* target, long F, float* E);
/* Per-frame figures of the Upper stage's epoch evaluation (Processor/Train/Train_Upper.py:75-88 angle_loss, :228-240):
 * U[f,0:15] error (m) of the 15 upper joints (upper_joint_map order), U[f,15:29] angles (deg) of the 14 upper-body bones,
 * U[f,29] sum |upper - target[upper_joint_map]| of the frame (its share of L1Loss(sum)).  upper [F,15,3], target [F,21,3], U [F,30]. */
int mmego_pose_errors_upper(void* stream, const float* upper, const float* target, long F, float* U);

/* ---- aligned evaluation metrics (metrics.hip; not in the reference) ------------------------------------
 * What mmego_pose_errors' absolute joint error mixes, taken apart per frame: the articulated pose against the placement of the whole
 * body by the head pose.  upper [F,15,3], lower [F,8,3] or NULL, target [F,21,3].  With `lower` the J = 21 joints are the skeleton as
 * mmego_pose_errors assembles it (lower overwrites the shared hips); with lower = NULL the J = 15 upper joints in upper_joint_map order
 * against target[:, upper_joint_map].  Root = joint 0 (spine base, position 0 of the upper map too).  The prediction p is fitted onto
 * the target g: minimise sum_j |s R (p_j - pbar) + gbar - g_j|^2 over PROPER rotations R (det = +1, never a reflection), s = 1 (rigid
 * fit) or the optimal s (similarity fit, Procrustes); pbar, gbar: centroids over the J joints.  Row A[f, :], lda >= width =
 * mmego_pose_errors_aligned_width(J, nthr) = 3 J + 3 + nthr:
 *   A[f, 0:J]     root-relative error per joint (m), |(p_j - p_0) - (g_j - g_0)|
 *   A[f, J:2J]    error per joint after the rigid fit
 *   A[f, 2J:3J]   error per joint after the similarity fit (PA-MPJPE per joint)
 *   A[f, 3J]      rotation angle of the fit (deg, in [0, 180]);  A[f, 3J+1] = |pbar - gbar| (m);  A[f, 3J+2] = the similarity scale s
 *   A[f, 3J+3+k]  fraction of the J joints whose ABSOLUTE error |p_j - g_j| is <= thr[k] (PCK); thr: nthr floats (m), 0 <= nthr <= 8
 * Horn's quaternion form, the eigenpair by a fixed number of cyclic Jacobi sweeps, s = lambda_max / sum_j |p_j - pbar|^2, the angle as
 * 2 atan2(|q_xyz|, |q_w|); all in double from the fp32 inputs, float stores; sums over the joints in index order (two launches give the
 * same bits).  A prediction without spread: s = 0, R = I, angle 0; a zero covariance: R = I; where the best rotation is not unique
 * (collinear joints) one maximiser is taken -- the sum of squared residuals is the same for all.  Means over frames via mmego_colsum. */
int mmego_pose_errors_aligned_width(int J, int nthr);
int mmego_pose_errors_aligned(void* stream, const float* upper, const float* lower, const float* target, long F, const float* thr,
                              int nthr, float* A, long lda);
/* Temporal quality of the same J joints: upper [B,T,15,3], lower [B,T,8,3] or NULL, target [B,T,21,3], T >= 3.  Acc[b, j] (row stride
 * lda >= J) = mean over t = 1 .. T-2 of |(p[t-1] - 2 p[t] + p[t+1]) - (g[t-1] - 2 g[t] + g[t+1])| of joint j, in m per frame^2: the
 * error of the second differences (acceleration error; jitter shows here and in no per-frame figure).  Double inside, summed in t
 * order, float stores. */
int mmego_pose_accel_errors(void* stream, const float* upper, const float* lower, const float* target, long B, int T, float* Acc,
                            long lda);

/* ---- eval-mode front end of Upper_Net in one launch (front.hip) ---------------------------------------
 * Per frame of N points (x [F,N,6], N a multiple of 16, <= 1024): Transform2H (Utils.py:284-292; bit-identical to mmego_transform2h,
 * written back into x -- quirk Q1 -- from x_src when given), PointNet 6-8-16-24 (Net/Upper_Net.py:242-266), concat with the first
 * four transformed columns, GlobalPointNet 28-32-48-64 and its softmax attention pooling (:270-301), all with eval-mode BatchNorm
 * folded into the k=1 convs.  vec [F,64] pooled features, attn [F,N] attention weights.  w: HOST array of 38 device pointers --
 * for PointNet conv1..3 then GlobalPointNet conv1..3: weight, bias, BatchNorm gamma, beta, running_mean, running_var; then the
 * attention Linear's weight [64] and bias [1].  Replaces transform2h + 2 x mlp3_eval + attn_pool_forward and their HBM round trips. */
int mmego_upper_front_eval(void* stream, float* x, const float* x_src, const float* R, const float* t, long F, int N,
                           const float* const* w, float eps, float* vec, float* attn);
/* A whole BiLSTM layer's recurrence for Bn <= 64 rows and H = 512 as ONE persistent launch with stationary weights (lstm_seq.hip;
 * IMU_Net's rnn_slow, Net/IMU_Net.py:61-62,82): xproj [Bn*T][xs >= 8H] rows (b*T + t) = W_ih x + b_ih of direction d at columns [4H d,
 * 4H d + 4H); out [Bn*T][os >= 2H]: h_t of direction d at columns [H d, H d + H); h_0 = c_0 = 0.  256 workgroups in 8 independent
 * groups (direction x 16 rows) that exchange h_t as (value, tag) words through xbuf.  sync: 16 unsigned words, xbuf: 2 * 8 * 16 * 512
 * 8-byte words, both zero before the first launch and private to one stream of launches; sync[9] is a sticky error flag (non-zero: a
 * bounded spin ran out -- the launch's workgroups could not all be resident -- and the results are invalid), sync[10] the launch
 * generation. */
/* mmego_lstm_seq_xcd_slots: how many such launches the current device holds at once (the 256 workgroups of a launch must be
 * co-resident): the kernel's occupancy (hipOccupancyMaxActiveBlocksPerMultiprocessor) x CU count / 256, per device -- 2 on a whole
 * MI355X, 0 on a device / partition too small for one launch.  mmego_lstm_seq_xcd_ok is 0 there too.  A caller that may have k such
 * launches in flight on different streams at once (two frozen IMU_Net forwards side by side) needs slots >= k. */
int mmego_lstm_seq_xcd_slots(void);
int mmego_lstm_seq_xcd_ok(int Bn, int H, int T);
int mmego_lstm_seq_xcd(void* stream, const float* xproj, long xs, const float* whh0, const float* whh1, const float* bhh0,
                       const float* bhh1, float* out, long os, unsigned* sync, unsigned long long* xbuf, int Bn, int H, int T);
/* The same launch with the six stages' operands (folded weights, activation tiles) rounded to bf16 and fp32 accumulation
 * (front_bf16.hip; opt-in precision mode of eval forwards).  Transform2H and its write-back stay fp32 and bit-identical. */
int mmego_upper_front_eval_bf16(void* stream, float* x, const float* x_src, const float* R, const float* t, long F, int N,
                                const float* const* w, float eps, float* vec, float* attn);

/* ---- fp32-accurate products on the bf16 matrix pipe ("split3", split3.hip) ------------------------------------
 * Opt-in mode of the frozen IMU_Net forward (Net/IMU_Net.py:58-62,76-83; IMUNet.precision = "split3"): every fp32 operand of the
 * BiLSTM products is split EXACTLY into three bf16 pieces a = a1 + a2 + a3 (round to nearest even, residuals exact) and a product
 * is the fp32-accumulated sum of the six piece products a1b1, a1b2, a2b1, a2b2, a1b3, a3b1 (nprod = 6; dropped terms <= 2^-24
 * relative) or of all nine (nprod = 9) on v_mfma_f32_32x32x16_bf16.
 * Operand layout "sfrag": block (rb, s, p) -- 32 rows x 16 k of piece p as the MFMA lanes read it, lane l = row 32 rb + l % 32,
 * k = 16 s + 8 (l / 32) .. + 8 -- is 1 KB at ((rb * K / 16 + s) * 3 + p) KB.  Activation rows are time-major (t * Bp + b). */
int mmego_split3_cvt(void* stream, const float* X, long ldx, long rows_in, int K, int tm, int Bn, int T, int Bp, long Rp,
                     unsigned short* Y);
/* mmego_split3_gemm cut into nsplit slabs of K (a long contraction with few output tiles): slab y leaves its partial product row-major
 * at ws + y * (32 Mrb) * (32 Nrb) floats -- the format mmego_slab_reduce kind 0 sums. */
int mmego_split3_gemm_slabs(void* stream, const unsigned short* A, const unsigned short* W, float* ws, int Mrb, int Nrb, int K,
                            int nprod, int wm, int nsplit);
/* out[i] = sum over y < nsplit of ws[y * n + i] (slab order): the K slabs of mmego_split3_gemm_slabs as one streaming sum.  n % 4 == 0. */
int mmego_split3_slab_sum(void* stream, const float* ws, int nsplit, long n, float* out);
/* The pieces of X^T for X [R][C] row-major (weight-gradient operands: both are read along the row axis): Y = sfrag of the [Cp x R]
 * matrix, Cp % 32 == 0 >= C, R % 16 == 0.  T > 0: column r of X^T is row r + shift of X where that row lies in the same T-row sequence
 * (rows b T + t), zero otherwise -- h_{t-1} / h_{t+1} of a layer's outputs without a shifted copy; T = 0, shift = 0: plain. */
int mmego_split3_cvt_t(void* stream, const float* X, long ldx, long R, int C, long Cp, unsigned short* Y, int shift, int T);
int mmego_split3_join(void* stream, const unsigned short* Y, long Rp, int K, float* X, long ldx);
int mmego_split3_fc_relu(void* stream, const float* X, long ldx, const float* W, const float* bias, int Bn, int T, int Cin,
                         int H, unsigned short* Y, int Bp, int relu);
int mmego_split3_gemm(void* stream, const unsigned short* A, const unsigned short* W, float* Cf, float* C, long ldc,
                      const float* bias, int Mrb, int Nrb, int K, int M, int nprod, int wm);
int mmego_split3_step(void* stream, int ndir, int Bn, int H, int first, const unsigned short* hprev0, const unsigned short* hprev1,
                      long hrb, const unsigned short* whh0, const unsigned short* whh1, const float* xpf, long mt0_0, long mt0_1,
                      float* hout0, float* hout1, long hos, unsigned short* hnext0, unsigned short* hnext1, long hnrb,
                      float* c0, float* c1, int nprod, int dbase);
/* projection for few rows (M <= 2048): C[m][d 4H + n] = A[m][:] . W_d[n][:] + bias[d 4H + n], both directions; W_d rows reordered
 * [32-unit block][gate][32 units]; K = 256 / 512 / 1024; C row-major (IMU_Net's rnn_slow: Net/IMU_Net.py:61-62,82) */
int mmego_split3_proj(void* stream, const unsigned short* A, const unsigned short* W0, const unsigned short* W1, const float* bias,
                      float* C, long ldc, int M, int H, int K, int nprod);
/* the same timestep on 16-unit workgroups (two per CU: single-direction launches of a layer's two directions run as two chains);
 * W_hh rows -- and the projection's columns -- ordered [16-unit block][gate][16 units] */
int mmego_split3_step16(void* stream, int ndir, int Bn, int H, int first, const unsigned short* hprev0, const unsigned short* hprev1,
                        long hrb, const unsigned short* whh0, const unsigned short* whh1, const float* xpf, long mt0_0, long mt0_1,
                        float* hout0, float* hout1, long hos, unsigned short* hnext0, unsigned short* hnext1, long hnrb,
                        float* c0, float* c1, int nprod, int dbase);

/* ---- anchor ("voxel") grouping of UpperNetwlocal (group.hip) -----------------------------------------
 * Per frame and per anchor of the 3x3x3 grid: indices (int64, exact, stable ties) of the 8 nearest points and
 * the gathered rows cat(anchor, xyz-anchor, features) -- square_distance / point_ball_set / AnchorGrouping of
 * Net/Upper_Net.py:10-32,54-72,100-119 (quirk Q5: points with xyz == 0 are at distance +inf).
 * xf rows hold xyz in columns 0:3 and D features after them; grouped is [F*27*8, 6+D]; dist_out may be NULL. */
int mmego_anchor_group(void* stream, const float* xf, long ldx, long F, int N, int D, const float* anchors,
                       long long* idx, float* grouped, float* dist_out);
/* Scatter the gradient of the gathered rows back to the points (accumulates into dxf, fixed order). */
int mmego_anchor_group_backward(void* stream, const float* dgrouped, const long long* idx, long F, int N, int D,
                                float* dxf, long lddx);

/* ---- the anchor ("voxel") branch of UpperNetwlocal, fused (local.hip): Net/Upper_Net.py:10-119,147-177,219-239 ---------------------
 * mmego_local_group_l1: per frame the 27 x N squared distances (reference rounding, Q5), the 8 nearest points of every anchor (int64
 * idx [F][27][8], stable ties) by wave-wide minimum rounds, the gathered rows cat(anchor, xyz - anchor, features) built in LDS and
 * multiplied there with LocalPointNet's first k=1 conv: Z1 [F*216][C1] = gathered W1^T + b1, part1[min(nwg, F)][2][64] = per-workgroup
 * (sum z, sum z^2) in fp64 (mmego_mlp_fwd_layer_n's in_part).  grouped (may be NULL) receives the gathered rows [F*216][6+D] (training:
 * the layer's weight gradient reads them); W1 NULL: grouping only.  N in {64, 128, 256}; 6 + D <= 32; C1 <= 32, C1 % 4 == 0.
 * mmego_pool8_bn_act: y = relu(BN(Z)) with the statistics finalized from mmego_mlp_fwd_layer's partials, attention score y.w + b,
 * softmax over each group's 8 rows -> attn [rows], pooled vectors -> voxT [F][64][27] (Conv3d input order); rows = F*27*8, C = 64.
 * mmego_pool8_backward: gradient of Z's activated rows dY from dvoxT [F][64][27] (y recomputed from Z and state [4][64]), gpart
 * [mmego_pool8_nblk(rows)][2][64] = (sum g, sum g xhat) with g = dY.[y > 0] (mmego_mlp_bwd_layer's g_part), awpart [nblk][128] =
 * per-workgroup partials of d(attention weight) [0:64] and d(bias) [64].
 * mmego_anchor_scatter: dxf[f][p][0:3+D] += sum over slots with idx == p of dgrouped[slot][3:6+D], slot order (deterministic). */
int mmego_local_group_l1(void* stream, const float* feats, long ldf, long F, int N, int D, const float* anchors, long long* idx,
                         float* grouped, const float* W1, const float* b1, int C1, float* Z1, long ldz1, double* part1, int nwg,
                         float* dist_out);
/* The eval-mode branch up to the pooled vectors in ONE launch: grouping, LocalPointNet's three conv + BatchNorm (running statistics,
 * folded) + ReLU stages, attention score, softmax over the 8 members, weighted sum; tab = HOST array of 20 device pointers: per layer
 * {W, b, gamma, beta, running_mean, running_var}, then the attention weight and bias.  Writes idx, attn [F*216], voxT [F][64][27]. */
int mmego_local_front_eval(void* stream, const float* feats, long ldf, long F, int N, int D, const float* anchors, long long* idx,
                           const float* const* tab, double eps, float* voxT, float* attn);
int mmego_pool8_nblk(long rows);
int mmego_pool8_bn_act(void* stream, const float* Z, long ldz, long rows, const double* part, const float* gamma, const float* beta,
                       double eps, float* rmean, float* rvar, double momentum, float* state, const float* aw_w, const float* aw_b,
                       float* voxT, float* attn);
int mmego_pool8_backward(void* stream, const float* Z, long ldz, long rows, const float* state, const float* attn, const float* dvoxT,
                         const float* aw_w, float* dY, long lddy, double* gpart, float* awpart);
int mmego_anchor_scatter(void* stream, const float* dgrouped, const long long* idx, long F, int N, int D, float* dxf, long lddx);
/* GlobalPointNet's softmax pooling over the 128 points of a frame (Upper_Net.py:285-301) fused the same way: forward = BatchNorm (from
 * mmego_mlp_fwd_layer's partials) + ReLU + score + softmax + weighted sum -> vec [F][64], attn [F*128] (the activated tensor is never
 * stored); backward = row gradients dY with y recomputed, gpart [rows/256][2][64] and awpart [rows/256][128] as mmego_pool8_backward.
 * rows = F * 128 with mmego_pool128_ok(rows) (two frames per workgroup = mlp_train's 256-row partition, rows <= 65 536). */
int mmego_pool128_ok(long rows);
int mmego_pool128_bn_act(void* stream, const float* Z, long ldz, long rows, const double* part, const float* gamma, const float* beta,
                         double eps, float* rmean, float* rvar, double momentum, float* state, const float* aw_w, const float* aw_b,
                         float* vec, float* attn);
int mmego_pool128_backward(void* stream, const float* Z, long ldz, long rows, const float* state, const float* attn, const float* vec,
                           const float* dvec, const float* aw_w, float* dY, long lddy, double* gpart, float* awpart);

/* ---- pooling / attention / graph (pool.hip) -------------------------------------------------------
 * Softmax-attention pooling over the P points of each of G groups (Upper_Net.py:285-301,163-177,
 * IMU_Net.py:79-80).  X [G, P, C] contiguous, w [C], b one float or NULL (0); vec [G, C], attn [G, P]; P <= 8192.
 * No operand has to be aligned; alignment only picks the kernel (tests/pool_ref.py mirrors the choice, tests/test_pool_kernels_gpu.py
 * runs every branch against float64):
 *   forward   C % 4 == 0 and X, w, vec on 16-byte addresses: the register kernel for P <= 32, C <= 1024, else the LDS kernel while
 *             its tile, (P C + P) * 4 bytes, is at most 96 KB; anything else -- C % 4 != 0, one of the three a float off, a larger
 *             tile -- takes the plain two-pass kernel.  attn is never read or written in 16-byte pieces.
 *   backward  C % 4 == 0, C < 256 dividing 256 or C >= 256, X on a 16-byte address and a tile, (P C + 2 P + PG C) * 4 bytes with
 *             PG = 256 / min(C, 256), of at most 64 KB: the LDS kernel; else the plain one.  w, attn, dvec, dX, pdw, pdb may lie
 *             anywhere.  attn is read as given (the forward's output); pdw [G, C] and pdb [G] are per-group partial gradients.
 *   Both tile limits are on the DYNAMIC LDS alone: each LDS kernel holds 8,224 bytes of static arrays on top (at most 104.5 KB and
 *   72.2 KB per workgroup of a CU's 160 KB), so the launchers raise the kernels' dynamic-LDS limit before they launch.
 * All kernels add in a fixed order: two launches on the same operands give the same bits; the kernels of one entry point agree to
 * rounding, not to the bit. */
int mmego_attn_pool_forward(void* stream, const float* X, const float* w, const float* b, long G, int P, int C,
                            float* vec, float* attn);
int mmego_attn_pool_backward(void* stream, const float* X, const float* w, const float* attn, const float* dvec, long G,
                             int P, int C, float* dX, float* pdw, float* pdb);
/* Y[g,:] = scale * sum_p X[g,p,:] and its broadcast backward (Lower_Net.py:112-115). */
int mmego_group_sum(void* stream, const float* X, long G, int P, int C, float scale, float* Y, long ldy);
int mmego_group_bcast(void* stream, const float* dY, long lddy, long G, int P, int C, float scale, float* dX,
                      int accumulate);
/* softmax(Q K^T * scale) V, 64 queries x 15 keys x 64 channels per frame (Lower_Net.py:105-109).  ldkv: row stride of K and V
 * (and of dK, dV) in floats -- K and V may be the column halves of one [rows, 128] buffer (to_k and to_v as one stacked product). */
int mmego_cross_attn_forward(void* stream, const float* Q, const float* K, const float* V, long F, float scale, float* O,
                             long ldo, float* P, long ldkv);
/* The eval-mode form (r06): osum[f][0..63] (row stride ldos) = the sum over frame f's 64 queries of the attention output -- what
 * Lower_Net.py:131-133 does with it next (gate == 1) -- added in ascending query order (the bits of mmego_group_sum2 over O); neither
 * O nor P is stored.  Q, K, V 16-byte aligned, ldkv % 4 == 0. */
int mmego_cross_attn_forward_pooled(void* stream, const float* Q, const float* K, const float* V, long F, float scale, float* osum,
                                    long ldos, long ldkv);
/* ... with the query projection of Lower_Net.py:100 inside: Q = X Wq^T + bq from the point features X [F * 64][ldx] (Wq [64][64], bq
 * [64]) is computed per frame on the matrix pipe and never stored.  X, Wq, bq, K, V 16-byte aligned, ldx % 4 == 0, ldkv % 4 == 0. */
int mmego_cross_attn_forward_pooled_q(void* stream, const float* X, long ldx, const float* Wq, const float* bq, const float* K,
                                      const float* V, long F, float scale, float* osum, long ldos, long ldkv);
int mmego_cross_attn_backward(void* stream, const float* Q, const float* K, const float* V, const float* P,
                              const float* dO, long lddo, long F, float scale, float* dQ, float* dK, float* dV, long ldkv);
/* Gradient of einsum('nkctv,kvw->nctw') wrt A (GCN.py:62).  Writes per-block partial sums
 * partial_ws[mmego_graph_dA_nblk(G)][K*V*V]; reduce them with mmego_colsum (scale = A gives the edge-importance gradient).
 * A, imp, dZ (all three or none): the einsum's input gradient dZ [G, V, K*C] from the same launch (what mmego_graph_mix
 * with backward = 1 computes, same bits).  ldz / lddz: row strides of Z / dZ in floats (column slices of wider buffers). */
int mmego_graph_dA_nblk(long G);
int mmego_graph_dA(void* stream, const float* Z, const float* dY, long G, int V, int K, int C, float* partial_ws,
                   const float* A, const float* imp, float* dZ, long ldz, long lddz);
/* ---- ST-GCN layer pieces (gcn.hip): Net/GCN.py:55-64 (graph convolution einsum), :108-122 (9x1 temporal convolution) --------
 * mmego_graph_mix: Y[f][w][c] = sum_k sum_v (A . importance)[k][v][w] X[f][v][k*C + c]  (backward = 0; X is z [F][V][K*C]), or the
 * input gradient Y[f][v][k*C + c] = sum_w (A . importance)[k][v][w] X[f][w][c] (backward = 1; X is dy [F][V][C]).
 * ldx: row stride of X in floats (X may be a column slice of a wider buffer; Y is dense).
 * stats (may be NULL; forward, F <= 1024): [C][F][3] BatchNorm partial records (V, mean, M2) of Y per frame and channel, for
 * mmego_bn_finalize -- the batch statistics of st_gcn.tcn[0] without a pass of their own over Y.
 * mmego_tconv: temporal convolution over rows (b, t, v) as an implicit GEMM, out[r][n] = bias[n] + sum_tap sum_k
 * act(X[r + (tap - taps/2) V][k]) Wp[(tap*Cout + n)*Cin + k], taps leaving the sequence contribute zero; act = ReLU(BatchNorm)
 * given by in_state [4][Cin] (mean, invstd, gamma*invstd, beta) or identity (NULL).  Wp: the conv weight re-packed by
 * mmego_tconv_pack (mode 0; the input gradient of the convolution is the same call with X = dY, Cin/Cout swapped, on the mode-1
 * pack).  act_out (may be NULL, needs in_state): [rows][Cin], receives act(X) -- what the backward pass keeps.  Cin % 4 == 0.
 * mmego_tconv_pack: W[co][ci][tap] -> [tap][co][ci] (mode 0) / [taps-1-tap][ci][co] (mode 1) / both, one behind the other (mode 2).
 * mmego_tconv_wgrad: dW[co][ci][tap] (+)= sum_r dY[r][co] Xa[r + (tap - taps/2) V][ci] (the convolution's weight gradient, no
 * unfolded operand); ws: mmego_tconv_wgrad_nsplit(...) * taps * Cout * Cin floats of partial tiles, added in a fixed order. */
int mmego_graph_mix(void* stream, const float* X, const float* A, const float* importance, float* Y, long F, int V, int K, int C,
                    int backward, float* stats, long ldx);
int mmego_tconv_pack(void* stream, const float* W, int Co, int Ci, int taps, int mode, float* Wp);
int mmego_tconv(void* stream, const float* X, long ldx, const float* in_state, const float* Wp, const float* bias, float* Y,
                long ldy, float* act_out, int B, int T, int V, int Cin, int Cout, int taps);
int mmego_tconv_wgrad_nsplit(int B, int T, int V, int Cin, int Cout, int taps);
int mmego_tconv_wgrad(void* stream, const float* dY, long lddy, const float* Xa, long ldx, float* ws, float* dW, int accumulate,
                      int B, int T, int V, int Cin, int Cout, int taps);
/* out[b][c][r] = in[b][r][c]: the (B,64,T,V)->(B,T,V,64) re-view of GCN.py:351-353 (quirk Q8). */
int mmego_transpose_batched(void* stream, const float* in, float* out, long Bn, int R, int C);
int mmego_mul(void* stream, const float* a, const float* b, float* out, long n);
int mmego_add(void* stream, const float* a, const float* b, float* out, long n);
/* The once-per-training-forward tick of a net: x[i] += 1 for the BatchNorm num_batches_tracked counters (one launch for all
 * layers; n may be 0) and, when seed_ctr is given, the next value of the dropout seed counter (mmego_lstm64_forward). */
int mmego_inc_i64(void* stream, long long* x, long n, unsigned long long* seed_ctr);

/* ---- inter-layer dropout of the LSTM stacks whose step kernels do not carry it (dropout.hip; IMU_Net training) -------
 * taken[0] = seed_ctr[0], then seed_ctr[0] takes the value mmego_inc_i64 would give it: one training forward's seed word, which
 * every mask of that forward and of its backward reads (the counter itself may move on in between). */
int mmego_seed_take(void* stream, unsigned long long* seed_ctr, unsigned long long* taken);
/* Y[r][c] = X[r][c] * m(r * cols + c), m = 0 or 1/(1-p): the mask mmego_lstm64_forward stores as drop_mask, from the same hash of
 * (LOGICAL element index r * cols + c, seed_word[0], salt), whatever ldx and ldy are.  Y may be X itself (same base and ldx == ldy: in place); operands that overlap in any
 * other way are refused.  No mask is stored: backward runs the same call on the gradient.  Needs 0 < p < 1, cols % 4 == 0, rows * cols < 2^32, ldx, ldy >= cols; 16-byte accesses when both
 * bases and both leading dimensions are multiples of 4 floats, dword accesses otherwise. */
int mmego_lstm_dropout(void* stream, const float* X, long ldx, float* Y, long ldy, long rows, long cols, float p,
                       const unsigned long long* seed_word, int salt);

/* ---- train-mode pointwise MLP layers, fused per layer (mlp_train.hip) -------------------------------------------------
 * k=1 conv -> BatchNorm (batch statistics) -> ReLU stages of Net/Upper_Net.py:242-301,147-177 and Net/Lower_Net.py:40-72 in
 * training.  Channel widths <= 64.  nblk = mmego_mlp_train_nblk(rows) workgroups per layer launch; statistics partials are
 * nblk x 2 x 64 doubles, dW partials nblk x 4096 floats.  A BatchNorm "state" is [4][C] floats: mean, invstd, gamma*invstd, beta.
 *   mmego_mlp_fwd_layer     Z = act(X) W^T + bias, act = ReLU(BatchNorm) of the layer below finalized from in_part (NULL: identity;
 *                           workgroup 0 stores in_state and updates in_rmean / in_rvar with in_momentum); out_part receives this
 *                           layer's (sum z, sum z^2).
 *   mmego_mlp_bn_act        Y = ReLU(BatchNorm(Z)) for the last stage, statistics finalized from part (state, running stats as above).
 *   mmego_mlp_bn_bwd_reduce part = (sum g, sum g xhat), g = dY . [BatchNorm(Z) > 0]: first reduction of a block's backward chain.
 *   mmego_mlp_bwd_layer     dz from (dY, Z, state, g_part); dgamma, dbeta; dX = dz W (NULL: skipped); gprev_part = the same
 *                           two sums for the layer below (Xin = its pre-BN z, in_state its BatchNorm; NULL in_state: Xin is the
 *                           plain layer input); dW_part = per-workgroup dz^T act(Xin).
 *   mmego_mlp_dw_reduce     dW_l = fixed-order sum of the nblk partials, up to three layers per launch. */
int mmego_mlp_train_nblk(long rows);
int mmego_mlp_fwd_layer(void* stream, const float* X, long ldx, long rows, int Cin, const double* in_part, const float* in_gamma,
                        const float* in_beta, double in_eps, float* in_rmean, float* in_rvar, double in_momentum,
                        float* in_state, const float* W, const float* bias, int Cout, float* Z, long ldz, double* out_part);
int mmego_mlp_fwd_layer_n(void* stream, const float* X, long ldx, long rows, int Cin, const double* in_part, int in_nblk,
                          const float* in_gamma, const float* in_beta, double in_eps, float* in_rmean, float* in_rvar,
                          double in_momentum, float* in_state, const float* W, const float* bias, int Cout, float* Z, long ldz,
                          double* out_part);
int mmego_mlp_bn_act(void* stream, const float* Z, long ldz, long rows, int C, const double* part, const float* gamma,
                     const float* beta, double eps, float* rmean, float* rvar, double momentum, float* state, float* Y,
                     long ldy);
int mmego_mlp_bn_bwd_reduce(void* stream, const float* dY, long lddy, const float* Z, long ldz, long rows, int C,
                            const float* state, double* part);
int mmego_mlp_bwd_layer(void* stream, const float* dY, long lddy, const float* Z, long ldz, long rows, int Cout,
                        const float* state, const double* g_part, float* dgamma, float* dbeta, const float* Xin, long ldxin,
                        int Cin, const float* in_state, const float* W, float* dX, long lddx, double* gprev_part,
                        float* dW_part);
/* mmego_mlp_bwd_layer for the first stage of LocalPointNet with its input rows GATHERED on the fly through the group indices (row r =
 * cat(anchors[(r % 216) / 8], xyz - anchor, features) of point gidx[r] of frame r / 216; feats [F*N][ldf] = xyz | D features): the
 * gathered tensor of mmego_local_group_l1 need not be kept for the layer's weight gradient. */
int mmego_mlp_bwd_layer_gather(void* stream, const float* dY, long lddy, const float* Z, long ldz, long rows, int Cout,
                               const float* state, const double* g_part, float* dgamma, float* dbeta, const long long* gidx,
                               const float* feats, long ldf, const float* anchors, int N, int D, const float* W, float* dX,
                               long lddx, float* dW_part);
int mmego_mlp_dw_reduce(void* stream, long rows, int nlayers, const float* part0, float* dW0, int Cout0, int Cin0,
                        const float* part1, float* dW1, int Cout1, int Cin1, const float* part2, float* dW2, int Cout2, int Cin2);
/* mmego_mlp_dw_reduce for up to 9 layers of several chains in ONE launch (descs: n MmegoDwRed; a layer's partials are
 * mmego_mlp_train_nblk(rows) x 4096 floats).  nblk > 0 / stride > 0 describe other per-workgroup partial records summed the same way:
 * nblk records `stride` floats apart, element (m, n) of a record at m * 64 + n (e.g. the pooling kernels' attention-parameter partials:
 * Cout = 1, Cin = 64, stride 128). */
typedef struct MmegoDwRed { const float* part; float* dW; int Cout, Cin; long rows; int nblk; long stride; } MmegoDwRed;
int mmego_mlp_dw_reduce_multi(void* stream, int n, const MmegoDwRed* descs);

/* ---- LocalVoxelNet training step (vox.hip): Net/Upper_Net.py:180-205 -------------------------------------------------------------
 * Conv3d(64, 96, k=3) over the whole 3x3x3 anchor grid (= a 1728 -> 96 map per frame), two 1x1x1 convs 96 -> 128 -> 64, a train-mode
 * BatchNorm3d + ReLU behind each, over rows = B*T frames: 4 forward + 5 backward launches, one wherever a BatchNorm needs every row's
 * statistics (mmego_vox_ok: the widths these kernels are built for, K = 1728, 2 <= rows <= 4096; other shapes take the generic
 * launches).  Forward statistics travel as (mean, M2) records [ceil(rows/16)][C] float pairs (rec*), finalized in the consumer's
 * prologue; workgroup 0 writes bn->state [4][C] = mean, invstd, a, b and the running statistics (bn: an MmegoBnRef whose rec / nrec /
 * rows_per_rec fields are ignored).  Backward sums travel as (sum g, sum g xhat) pairs per 16-row tile (prt*).
 *   vox_l1_fwd    Z[rows][C] = X[rows][K] W[C][K]^T + bias, rec
 *   vox_mid_fwd   Yin = relu(bn(Zin)) [rows][Cin] (stored for backward), Zout = Yin W[Cout][Cin]^T + bias, rec_out; (Cin, Cout) = (96, 128), (128, 64)
 *   vox_out_fwd   Y[rows][C] (row stride ldy) = relu(bn(Z))
 *   vox_bwd_sums  G = dY . [Y > 0] [rows][C], prt from Z and the forward state
 *   vox_mid_bwd   dZ = BatchNorm backward of G (sums prt, state; dgamma / dbeta assigned), Gp = (dZ W[Cout][Cin]) . [Yp > 0], prtp from Zp / statep;
 *                 (Cout, Cin) = (64, 128), (128, 96)
 *   vox_l1_bwd    dZ as above for the first layer (C = 96), dX[rows][K] = dZ W[C][K]
 *   vox_dw        dW1[C1][K] = dZ1^T X, dW2[C2][C1] = dZ2^T Y1, dW3[C3][C2] = dZ3^T Y2 (assigned)
 * The conv biases get no gradient (exactly zero in front of a batch-statistics BatchNorm). */
struct MmegoBnRef;                 /* (defined with the fused ST-GCN step below) */
int mmego_vox_ok(long rows, int K, int C1, int C2, int C3);
int mmego_vox_l1_fwd(void* stream, const float* X, long ldx, long rows, int K, const float* W, const float* bias, int C, float* Z,
                     float* rec);
int mmego_vox_mid_fwd(void* stream, const float* Zin, const float* rec_in, const struct MmegoBnRef* bn, long rows, int Cin, float* Yin,
                      const float* W, const float* bias, int Cout, float* Zout, float* rec_out);
int mmego_vox_out_fwd(void* stream, const float* Z, const float* rec, const struct MmegoBnRef* bn, long rows, int C, float* Y, long ldy);
int mmego_vox_bwd_sums(void* stream, const float* dY, long lddy, const float* Y, long ldy, const float* Z, const float* state,
                       long rows, int C, float* G, float* prt);
int mmego_vox_mid_bwd(void* stream, const float* G, const float* Z, const float* state, const float* prt, long rows, int Cout,
                      float* dZ, float* dgamma, float* dbeta, const float* W, int Cin, const float* Yp, const float* Zp,
                      const float* statep, float* Gp, float* prtp);
int mmego_vox_l1_bwd(void* stream, const float* G, const float* Z, const float* state, const float* prt, long rows, int C, float* dZ,
                     float* dgamma, float* dbeta, const float* W, int K, float* dX, long lddx);
int mmego_vox_dw(void* stream, long rows, const float* dZ1, const float* X, long ldx, float* dW1, int C1, int K, const float* dZ2,
                 const float* Y1, float* dW2, int C2, const float* dZ3, const float* Y2, float* dW3, int C3);

/* ---- fused ST-GCN training step (gcn_fused.hip, gcn.hip): Net/GCN.py:67-147 st_gcn, :332-355 Model.extract_feature -----------------
 * Train-mode BatchNorm statistics travel between these kernels as PARTIAL RECORDS: per producer workgroup j and channel c the float
 * pair rec[j][c] = (mean_j, M2_j) over the rows the workgroup owns (rows_per_rec each, the last record ragged).  The consumer finalizes
 * them in its prologue (every workgroup, fixed order); workgroup 0 writes state [4][C] = mean, invstd, a, b and updates the running
 * statistics with torch semantics.  Replaces the colstats / bn_finalize / affine_act launches between the products. */
typedef struct MmegoBnRef {
  const float* rec; int nrec; int rows_per_rec;
  const float* gamma; const float* beta; float* running_mean; float* running_var; float momentum; float eps;
  float* state;
} MmegoBnRef;
/* One launch per st_gcn block front: [in_mode 1: x = relu(bn1(X1) + bn2(X2)), both BatchNorms from records | in_mode 0: x =
 * data_bn(X1), X1 = the frame tensor [F][V*cin], statistics computed by the kernel itself (F <= 1024)] -> xact [F*V][cin] (kept for
 * backward; may be NULL) -> zr = x W^T + bias, W [nout][cin] the stacked weight of the graph convolution's and the residual branch's
 * 1x1 convs -> mix = 1: Z [F*V][(K+1) cout] = zr, Y [F*V][cout] = einsum('nkctv,kvw->nctw', z, A . importance), recY / recR
 * [mmego_gcn_front_nrec(F)][cout]: records of Y and of the residual columns of Z (4 frames = 4 V rows per record); mix = 0: the
 * closing 1x1 conv, stored transposed outT[b][nout][T*V] (GCN.py:351-353, the re-viewed layout).  cin in {<32 with in_mode 0, 32,
 * 64, 128}; nout a multiple of 32 (<= 384 with cin <= 64; in_mode 0: cin <= 8, nout <= 128 and nout * cin <= 512); mix = 1 with
 * cin >= 32: cout in {32, 64, 128}. */
typedef struct MmegoGcnFront {
  const float* X1; long ld1; const float* X2; long ld2; int in_mode;
  MmegoBnRef bn1, bn2;
  float* xact;
  const float* W; const float* bias; int cin, nout;
  int mix, K, cout; const float* A; const float* importance;
  float* Z; long ldz; float* Y; float* recY; float* recR;
  float* outT; int T;
  long F; int V;
} MmegoGcnFront;
int mmego_gcn_front_nrec(long F);
int mmego_gcn_front(void* stream, const MmegoGcnFront* desc);
/* mmego_tconv in the fused training step: in_bn = MmegoBnRef of the BatchNorm (+ReLU) in front, out_rec [ceil(rows/64)][Cout] =
 * records of the output for the BatchNorm behind; mmego_tconv_bwd_stats = the input-gradient call (X = dY, gradient pack) whose
 * epilogue leaves bw_rec [ceil(rows/64)][Cout] = (sum g, sum g xhat), g = dAct . [bn(ymix) > 0], for the BatchNorm + ReLU in front of
 * the convolution's input (state [4][Cout]).  mmego_pack_multi: every weight re-layout of a step in one launch, n <= 8 entries -- kind 0:
 * mmego_tconv_pack mode 2 of W[Co][Ci][taps]; kind 1: a k=1 conv weight W[Co][Ci] (both multiples of 32) in the FRAGMENT-MAJOR order
 * mmego_gcn_front reads with one coalesced 1-KB fetch per MFMA operand group (gcn.hip, pack_multi_kernel) -- MmegoGcnFront.W then
 * points at that copy when cin >= 32. */
int mmego_tconv_train(void* stream, const float* X, long ldx, const MmegoBnRef* in_bn, const float* Wp, const float* bias, float* Y,
                      long ldy, float* act, float* out_rec, int B, int T, int V, int Cin, int Cout, int taps);
int mmego_tconv_bwd_stats(void* stream, const float* dY, long lddy, const float* Wp, float* dAct, long ldda, const float* ymix,
                          long ldym, const float* state, float* bw_rec, int B, int T, int V, int Cin, int Cout, int taps);
/* Sequence-tiled forms of the two calls above for T*V <= 127 rows per sequence and Cin in {32, 64, 128} (mmego_tconv_seq_ok): one
 * workgroup per (sequence, 32 output columns), the sequence's rows staged in LDS once for all taps, weights Wf fragment-major per tap
 * (mmego_pack_multi kind 2: 2 * taps * Co * Ci floats, the forward image then the input-gradient image); out_rec / bw_rec are per
 * SEQUENCE: [B][Cout], T*V rows per record. */
int mmego_tconv_seq_ok(int T, int V, int Cin, int Cout);
int mmego_tconv_seq_train(void* stream, const float* X, long ldx, const MmegoBnRef* in_bn, const float* Wf, const float* bias, float* Y,
                          long ldy, float* act, float* out_rec, int B, int T, int V, int Cin, int Cout, int taps);
int mmego_tconv_seq_bwd(void* stream, const float* dY, long lddy, const float* Wf, float* dAct, long ldda, const float* ymix,
                        long ldym, const float* state, float* bw_rec, int B, int T, int V, int Cin, int Cout, int taps);
/* Eval-mode ST-GCN block with bf16 operands and fp32 accumulation (opt-in precision mode; csrc/gcn_bf16.hip; reference
 * Net/GCN.py:55-64,67-147 with the BatchNorms frozen).  A block = mmego_gcn_mix_eval_bf16 + mmego_tconv_eval_bf16:
 *   gcn_mix: Yact = bf16(relu(bn0(einsum(conv1x1(X), A . importance)))), Rn = bn_r(residual conv1x1(X)) in fp32; the einsum is applied
 *     to X in fp32 in front of the product (exact in real arithmetic), the product's k axis is [A_0^T X | A_1^T X | A_2^T X | X].
 *     Wy / Wr: the two weights in bf16, fragment-major [Cout / 32][k steps][64 lanes][8] with lane (n, hf) of step ks holding
 *     W[32 ct + n][16 ks + 8 hf .. + 8] over the k axis above (Wy: rows of the graph conv, zero over X's columns, steps [0, ksy);
 *     Wr: the residual conv, zero elsewhere, steps [kr0, kr0 + ksr); ksy = ceil(K Cin / 16), kr0 = floor(K Cin / 16), kr0 + ksr =
 *     ceil((K + 1) Cin / 16)); biasy [V][Cout] = sum_k
 *     colsum_v((A . importance)[k])[w] b_k[c]; in_state: [4][V Cin] state of data_bn applied while loading (first block) or NULL;
 *     st0 / st_r: [4][Cout] mean, invstd, a, b.
 *   tconv: Y = relu?(bn?(bias + temporal conv of X (bf16, activated)) + res); Wp from mmego_tconv_pack_bf16 (taps * Cout * Cin bf16);
 *     one workgroup per sequence, (T + taps - 1) V rows of LDS (mmego_tconv_eval_bf16_ok). */
int mmego_gcn_mix_eval_bf16_ok(int V, int Cin, int Cout, int K);
int mmego_gcn_mix_eval_bf16(void* stream, const float* X, const float* in_state, const float* A, const float* importance,
                            const unsigned short* Wy, const unsigned short* Wr, const float* biasy, const float* biasr,
                            const float* st0, const float* st_r, unsigned short* Yact, float* Rn, long F, int V, int Cin, int Cout,
                            int K);
int mmego_tconv_eval_bf16_ok(int T, int V, int Cin, int Cout, int taps);
int mmego_tconv_eval_bf16(void* stream, const unsigned short* X, const unsigned short* Wp, const float* bias, const float* post,
                          const float* res, long ldr, float* Y, long ldy, int relu, int B, int T, int V, int Cin, int Cout, int taps);
int mmego_tconv_pack_bf16(void* stream, const float* W, int Cout, int Cin, int taps, unsigned short* Wp);
typedef struct MmegoPack { const float* W; float* Wp; int Co, Ci, taps, kind; } MmegoPack;
int mmego_pack_multi(void* stream, int n, const MmegoPack* descs);
/* Backward of a block's closing pair out = relu(BN(X1) + BN(X2)) (same dY, mask = out): reduce -> rec [ceil(rows/64)][2C] (sum g, sum
 * g xhat), virtual channels [0, C) = first BatchNorm, [C, 2C) = second; apply: finalize in the prologue, dX = a (g - mean(g) - xhat
 * mean(g xhat)) for both, d(gamma) / d(beta) by workgroup 0.  st1 / st2: state [4][C].  C % 4 == 0, C <= 128. */
int mmego_gcn_bn_bwd_reduce(void* stream, const float* dY, long lddy, const float* mask, long ldm, const float* X1, long ld1,
                            const float* st1, const float* X2, long ld2, const float* st2, long rows, int C, float* rec);
int mmego_gcn_bn_bwd_apply(void* stream, const float* dY, long lddy, const float* mask, long ldm, const float* X1, long ld1,
                           const float* st1, const float* X2, long ld2, const float* st2, long rows, int C, const float* rec,
                           float* dgamma1, float* dbeta1, float* dX1, long lddx1, float* dgamma2, float* dbeta2, float* dX2,
                           long lddx2);
/* mmego_graph_dA with the backward of the BatchNorm + ReLU behind the einsum applied on load: dY0 = gradient of the activated rows,
 * Ymix = the einsum output (pre-BatchNorm), st0 = that BatchNorm's state, rec [nrec][C] = mmego_tconv_bwd_stats' records; writes
 * d(gamma), d(beta), the dA partials [mmego_graph_dA_fused_nblk(G)][K*V*V] and dZ. */
int mmego_graph_dA_fused_nblk(long G);
int mmego_graph_dA_fused(void* stream, const float* Z, long ldz, const float* dY0, const float* Ymix, const float* st0,
                         const float* rec, int nrec, float* dgamma0, float* dbeta0, long G, int V, int K, int C,
                         float* partial_ws, const float* A, const float* imp, float* dZ, long lddz);
/* ONE launch for the deferred partial-product sums of a backward pass (fixed order).  kind 0: split-K slabs ws[nsplit][M*N] ->
 * out[m*scm + n] (what mmego_gemm leaves with accumulate = 2; asum != NULL: the slab row sums ws[nsplit*M*N + k*M + m] -> asum[m]);
 * kind 1: mmego_tconv_wgrad's slabs (accumulate = 2) ws[nsplit][taps][Co][Ci] -> out[co][ci][tap], M = taps*Co, N = Ci; kind 2:
 * out[i] = scale[i] * sum_k ws[k][i], M = 1 (edge-importance gradient from mmego_graph_dA's partials).  n <= 24. */
typedef struct MmegoSlab {
  const float* ws; float* out; const float* scale; float* asum;
  int kind, nsplit, M, N, taps; long scm;
} MmegoSlab;
/* Launch-count helpers of the Lower_Net tail: two group sums / two group broadcasts / two 2-D copies per launch, and mmego_topk_rows
 * with the kept rows' first n2 columns written to a second buffer as well (same arithmetic as the single forms). */
int mmego_transform2h_pair(void* stream, float* pts, long F, int P, int C, const float* R, const float* t, float* pts2, int P2,
                           const float* src2);
int mmego_colsum2(void* stream, const float* X1, long ld1, long rows1, int C1, float* out1, const float* X2, long ld2, long rows2,
                  int C2, float* out2);
int mmego_group_sum2(void* stream, long G, const float* X1, int P1, int C1, float scale1, float* Y1, long ldy1, const float* X2, int P2,
                     int C2, float scale2, float* Y2, long ldy2);
int mmego_group_bcast2(void* stream, long G, const float* dY1, long lddy1, int P1, int C1, float scale1, float* dX1, const float* dY2,
                       long lddy2, int P2, int C2, float scale2, float* dX2);
int mmego_copy2d_pair(void* stream, const float* X1, long ldx1, float* Y1, long ldy1, long rows1, int C1, const float* X2, long ldx2,
                      float* Y2, long ldy2, long rows2, int C2);
int mmego_topk_rows2(void* stream, const float* pts, long F, int N, int C, int keep, float* out, long long* idx, float* out2, long ld2,
                     int n2);
int mmego_slab_reduce(void* stream, int n, const MmegoSlab* descs);
/* d(gamma)[c] = sum_r dY[r][c] xhat[r][c], d(beta)[c] = sum_r dY[r][c] of a BatchNorm whose input gradient is not needed (data_bn,
 * GCN.py:310: the skeleton input is detached, Train_Lower.py:196); state [4][C]. */
int mmego_bn_param_grads(void* stream, const float* dY, long lddy, const float* X, long ldx, const float* state, long rows, int C,
                         float* dgamma, float* dbeta);
/* Input gradient of a train-mode BatchNorm from its finished parameter gradients: dX[r][c] = a[c] (dY[r][c] - dbeta[c] / rows -
 * xhat[r][c] dgamma[c] / rows), with dgamma / dbeta as mmego_bn_param_grads left them (the two column sums the formula needs: read,
 * not written).  data_bn when the predicted skeleton is differentiable (Lower_Net input gradients). */
int mmego_bn_input_grad(void* stream, const float* dY, long lddy, const float* X, long ldx, const float* state, long rows, int C,
                        const float* dgamma, const float* dbeta, float* dX, long lddx);

/* ---- optimiser (optim.hip) -------------------------------------------------------------------------
 * torch.optim.Adam step (coupled L2 weight decay) over one flat buffer; state = 3 doubles on the device
 * {step, lr/(1-b1^t), sqrt(1-b2^t)}, advanced by the call itself so a captured graph replays correctly
 * (Train_Upper.py:60,182; Train_IMU.py:71-72).  skip: HOST array of nskip (<= 4) [begin, end) element ranges (multiples of 4) that
 * the update leaves untouched -- parameters that never receive a gradient (torch.optim.Adam skips grad=None: IMU_Net.fc3,
 * Net/IMU_Net.py:55, which would otherwise decay under Train_IMU's weight_decay).  NULL / 0: update everything.
 * ticket: one device int, 0 before the first call and left 0 by every call (the step count in `state` advances inside the update
 * launch: the workgroup that finishes last stores it). */
int mmego_adam_step(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                    double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip, int* ticket);
/* Global-norm gradient clipping (clip_grad_norm_ ahead of the optimiser step), as two launches without a host read.
 * mmego_grad_norm_nblk: how many partial records mmego_grad_sqnorm writes for n floats (a function of n alone, <= 2048; pure host
 * helper).  mmego_grad_sqnorm: part[b] = the fp64 sum of workgroup b's g[i]^2 (each product formed in fp64), the skip ranges -- same
 * HOST array and checks as mmego_adam_step -- left out; the order of summation depends on n alone.  npart must equal
 * mmego_grad_norm_nblk(n).
 * mmego_adam_step_clipped: mmego_adam_step with every gradient element multiplied (fp32, rounded once) by
 * cf = (float)min(1, max_norm / (norm + 1e-6)), norm = sqrt(sum of part[0..npart)) in double; weight decay is added to the clipped
 * gradient.  A non-finite norm skips the step: p, m, v and state stay bit for bit, the step count does not advance.  max_norm > 0;
 * +inf never clips.  stats: 8 device doubles kept by the call {this step's norm, sum of finite norms, their maximum, steps seen,
 * steps with cf < 1, steps skipped as non-finite, reserved, reserved}. */
int mmego_grad_norm_nblk(long n);
int mmego_grad_sqnorm(void* stream, const float* g, long n, const long* skip, int nskip, double* part, int npart);
int mmego_adam_step_clipped(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                            double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip, int* ticket,
                            const double* part, int npart, double max_norm, double* stats);
/* The two steps above with an exponential moving average of the weights kept in the same launch (csrc/optim.hip, EMA).  The Adam part
 * is the plain one: the same p, g, m, v, state give the same bits in p, m, v, state (and stats, and the same ticket behaviour) as
 * mmego_adam_step / mmego_adam_step_clipped.  ema: n device floats, 16-byte aligned, not overlapping p; for every element the update
 * touches, ema = fmaf(omd, p_new - ema, ema) in fp32 with omd = (float)(1 - ema_decay) and p_new the parameter just stored.  Elements
 * inside a skip range keep their ema bit for bit, and so does every element of a step that the clipped form skips as non-finite.
 * 0 < ema_decay < 1 (NaN is refused); a refused call launches nothing. */
int mmego_adam_step_ema(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                        double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip, int* ticket,
                        float* ema, double ema_decay);
int mmego_adam_step_clipped_ema(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                                double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip, int* ticket,
                                const double* part, int npart, double max_norm, double* stats, float* ema, double ema_decay);

/* ---- learning-rate schedule inside the step (optim.hip, SCHED) -------------------------------------
 * The four steps above with the rate computed by the launch itself from the step count, so that a captured graph replays another
 * rate every step and a step skipped as non-finite consumes no schedule step.  With t = state[0] + 1 the step about to be taken,
 * all in double:
 *   w = t / W where W > 0 and t < W, else exactly 1;  s = max(0, t - W);  x = min(s, D) / D;
 *   d = 1 (constant) | r + (1 - r)(1 + cos(pi x)) / 2 (cosine) | r + (1 - r)(1 - x) (linear) | max(r, g^floor(s / E)) (step),
 *   d exactly 1 where s == 0;   lr_t = lr * (w * d);   from there the step is the one above at lr_t, bit for bit.
 * state: FOUR device doubles {t, lr_t / (1 - b1^t), sqrt(1 - b2^t), lr_t}, 8-byte aligned; state[3] is the rate of the last step taken.
 * part == NULL (then npart 0, stats NULL): the plain step, else the clipped one; ema == NULL (then ema_decay 0): no weight average.
 * sched: a HOST struct, copied into the kernel arguments.  Refused (nothing is launched): whatever the corresponding entry point
 * above refuses, sched == NULL, kind outside 0..3, reserved != 0, W negative / fractional / not finite, for cosine and linear D < 1 /
 * fractional / not finite, r outside [0, 1), for step E < 1 / fractional / not finite or g outside (0, 1].
 * (Declared as a tagged struct with its typedef behind it: hip.parse_tagged_structs reads this form.) */
struct MmegoLrSchedule {
  int kind;          /* 0 constant, 1 cosine, 2 linear, 3 step */
  int reserved;      /* 0 */
  double warmup;     /* W >= 0, integer-valued: optimiser steps of linear warm-up (0: none) */
  double span;       /* D >= 1, integer-valued: steps the decay takes behind the warm-up (cosine, linear) */
  double floor;      /* r in [0, 1): the decay's end value as a fraction of lr (step: its lower bound) */
  double every;      /* step: E >= 1, integer-valued */
  double gamma;      /* step: g in (0, 1] */
};
typedef struct MmegoLrSchedule MmegoLrSchedule;
int mmego_adam_step_sched(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                          double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip, int* ticket,
                          const double* part, int npart, double max_norm, double* stats, float* ema, double ema_decay,
                          const MmegoLrSchedule* sched);

/* ---- shaped weight decay inside the step (optim.hip, DECAY) ----------------------------------------
 * Every option of the steps above in one entry point, plus a mask of what decays and the decoupled (AdamW) form.  The arguments
 * are mmego_adam_step_sched's with its conventions (part == NULL: not clipped, ema == NULL: no average); sched == NULL selects the
 * unscheduled step (state: three doubles), else state has four.
 * decay_mask: one bit per float4 of the flat buffer in 64-bit words, word w bit b covering float4 64 w + b: (n / 4 + 63) / 64 device
 * words, 8-byte aligned, read only; bits beyond n / 4 in the last word are ignored.  NULL: every element decays.  An element whose
 * bit is clear is updated as with weight_decay = 0; an element inside a skip range is untouched whatever its bit.
 * decoupled == 0: where the bit is set the gradient of the update is g + weight_decay * p (g * cf under clipping), as in the steps
 * above -- with a NULL or all-set mask the call is bit for bit the corresponding entry point above.
 * decoupled == 1: with lr_t the rate of this step (the scheduled one where sched is given) and dw = (float)(lr_t * weight_decay),
 * the product formed in double, where the bit is set p' = fmaf(-dw, p, p) -- p - dw p rounded ONCE, not p * (1 - dw) -- and the
 * Adam update then runs on p' with the gradient alone: from p' the step is the one above at weight_decay = 0, bit for bit.  The
 * clip factor scales the raw gradient only, a step skipped as non-finite decays nothing, ema takes the final parameter.
 * Refused (nothing is launched): whatever mmego_adam_step_sched refuses (but a NULL sched), a decay_mask off an 8-byte boundary,
 * weight_decay negative, infinite or NaN, decoupled outside {0, 1}. */
int mmego_adam_step_decay(void* stream, float* p, const float* g, float* m, float* v, long n, double* state, double lr,
                          double beta1, double beta2, double eps, double weight_decay, const long* skip, int nskip, int* ticket,
                          const double* part, int npart, double max_norm, double* stats, float* ema, double ema_decay,
                          const MmegoLrSchedule* sched, const unsigned long long* decay_mask, int decoupled);

#ifdef __cplusplus
}
#endif
#endif
