// nnr_density_setup_f16.inc -- what a density-only kernel on the two-term fp16 trunk (nnr_trunk_f16.h) does before its first pass, as a block of
// statements at the top of the kernel's body: the LDS carve-up, the table load, the weight stream.  Included by march_f16_kernel, propose_f16_kernel
// and grid_f16_kernel; the pass itself is nnr_density_pass_f16.inc.  Names it takes from the including scope:
//   D                                        the kernel's template argument (the trunk's width)
//   a.packed                                 the packed weights of nnr_pack (Layout<D, 3>)
//   kDensityExtraF4                          constexpr int, defined in front of the include: f32x4 the kernel wants for itself between the park
//                                            area and the tables (0, or the proposal kernel's staging rows)
// Names it leaves behind:
//   L = Layout<D, 3>, Pipe, DT, HT           the layout, the weight stream's type, the tile counts
//   lane0, wave, wave_u                      the lane, the wave, the wave as a scalar
//   smem, kRingF4, kPark                     LDS in f32x4, in this order: the weight ring [0, kRingF4), the park area [kRingF4, + kPark: per wave 8
//                                            slots of 64 lanes), the kernel's extra [kRingF4 + kPark, + kDensityExtraF4), the tables
//   ltab                                     the bias / head / scale tables in LDS, loaded and behind a workgroup barrier
//   pipe                                     the weight stream, ending in front of the colour panels (n_panels = L::fwd_panel0(F_RGBH_F)), not started:
//                                            the kernel sets pipe.more from its pass count and calls pipe.start()
    using L = Layout<D, 3>;
    using Pipe = Split2PipeT<false>;
    constexpr int kRingF4 = kNBuf * Pipe::F4;
    constexpr int DT = L::DT, HT = L::HT;
    const int lane0 = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    constexpr int kPark = kWavesPerBlock * 8 * 64;   // per wave 8 16-byte slots per lane: the packed terms of posenc
    __shared__ __attribute__((aligned(16))) f32x4 smem[kRingF4 + kPark + kDensityExtraF4 + (L::table_floats + 3) / 4];
    float* const ltab = reinterpret_cast<float*>(smem + kRingF4 + kPark + kDensityExtraF4);
    for (int i = threadIdx.x; i < L::table_floats; i += 256) ltab[i] = a.packed[L::bias_base + i];
    __syncthreads();
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    Pipe pipe{reinterpret_cast<const f32x4*>(a.packed) + wave_u * (Pipe::PW * 64), smem, wave_u, lane0, L::fwd_panel0(F_RGBH_F)};
