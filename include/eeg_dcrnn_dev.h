/*
 * eeg_dcrnn_dev.h — DEVELOPMENT entry points, exported only by the dev build of the library
 * (`make -C eeg_gnn_ssl_amd/csrc dev` -> libeeg_dcrnn_hip_dev.so, compiled with -DEEG_DEV) and by the
 * test emulator.  The product library libeeg_dcrnn_hip.so does not export them: its kernel-variant
 * choices are compile-time constants and it carries no process-global mutable tuning state.
 * Users: tools/ (A/B timing, cycle probe) and `bench.py --tune`.
 */
#ifndef EEG_DCRNN_DEV_H
#define EEG_DCRNN_DEV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* When set to a device buffer of B*4*32 int64, the recurrent kernels store the shader-clock cycles each
 * wave spent per phase (slots 0-7 forward, 8-15 backward); NULL disables.  Only the H=64, M=3
 * instantiations carry the probe. */
int eeg_dcrnn_set_seq_probe(int64_t* probe);
/* Integer knobs selecting kernel variants for A/B timing; the keys are named below.  Defaults (all 0) = the product configuration. */
int eeg_dcrnn_set_tuning(int key, int value);
enum {
    /* the hoisted GEMMs (the inputs of the launch plans, csrc/gemm_launch.h) */
    EEG_TUNE_NN_STAGED = 0,          /* 1: register-staged NN GEMM */
    EEG_TUNE_TN_STAGED = 1,          /* 1: register-staged TN GEMM */
    EEG_TUNE_QUAD = 2,               /* bit 0: no persistent quad NN GEMM; bit 1: no quad TN GEMM; bits 2..: rows per CU from which they run */
    EEG_TUNE_TN_XCD = 4,             /* 1: NO XCD-aware placement of the TN k-blocks in the LDS-DMA kernel; 2: placement in the register-staged one */
    EEG_TUNE_TN_WIDE_FROM = 14,      /* 8-wave TN GEMM from this dY width up */
    EEG_TUNE_TN_TARGET = 15,         /* workgroup target of the split TN GEMMs */
    EEG_TUNE_TNQ_TARGET = 16,        /* workgroup target of the quad TN GEMM */
    EEG_TUNE_TN_NO_PAIR = 19,        /* 1: the two h-part weight-gradient GEMMs of a cell as two launches instead of the paired one */
    /* the recurrent kernels (the inputs of the launch plans, csrc/seq_launch.h) */
    EEG_TUNE_SEQ_STREAM = 3,         /* streamed-weight BPTT kernel, two workgroups per CU: 1 = wherever it exists, 2 = never */
    EEG_TUNE_SEQ_FWD_ONE_WAVE = 12,  /* 1: single-wave-per-SIMD forward kernel also where the two-wave one exists */
    EEG_TUNE_SEQ_BWD_ONE_WAVE = 13,  /* 1: the same for the BPTT kernel */
    EEG_TUNE_SEQ_BWD_NO_SPEC = 21,   /* 1: the general-path BPTT kernel under the spectral form */
    EEG_TUNE_SEQ_FWD_NO_SPEC = 22,   /* 1: the general-path forward kernel under the spectral form */
    /* diffusion, decoder, spectral form */
    EEG_TUNE_DIFFUSE_FWD_WGS = 5,    /* target workgroup count of the streaming diffusion, forward */
    EEG_TUNE_DIFFUSE_ADJ_WGS = 6,    /* the same, adjoint */
    EEG_TUNE_GRAM_WGS = 7,           /* the same, correlation-Gram launches */
    /* 8: unused (rounds 1-3: k-steps per weight group of the layer-0 input part in the persistent decoder forward) */
    EEG_TUNE_DIFFUSE_ADJ_LDS = 9,    /* 1: LDS/MFMA adjoint diffusion */
    EEG_TUNE_DEC_BWD_PER_STEP = 10,  /* 1: per-step launches in the decoder backward instead of the persistent kernel (read by the decoder plan, csrc/dec_launch.h) */
    EEG_TUNE_DEC_FWD_PER_STEP = 11,  /* 1: the same for the decoder forward */
    EEG_TUNE_SPEC_DX_PASSES = 17,    /* 1: input gradient of a spectral layer as grouped GEMM + node-mix pass instead of gemm_dxf_kernel (read by the spectral plan, csrc/spec_launch.h) */
    EEG_TUNE_DIFFUSE_ADJ_PLANES = 18, /* 1: the round-4 adjoint diffusion (hop planes one at a time) instead of the row-streaming one */
    EEG_TUNE_SPEC_NN_GROUPED = 20,   /* 1: the round-5 grouped NN GEMM for the spectral x-part instead of gemm_nnf_kernel (read by the spectral plan) */
    EEG_TUNE_SPEC_TN_SEPARATE = 23,  /* 1: the three grouped weight-gradient launches instead of the fused one (read by the spectral plan) */
    EEG_TUNE_COUNT = 24
};

#ifdef __cplusplus
}
#endif
#endif /* EEG_DCRNN_DEV_H */
