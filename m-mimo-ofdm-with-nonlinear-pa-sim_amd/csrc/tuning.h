// Build-time A/B switches of the fused trial kernel, in one place.
//
// Each switch selects between two implementations that give identical per-trial counts; the
// default is the one that measured faster in an interleaved A/B on one MI355X (tools/ab_libs.py;
// the records are under profiles/, DESIGN.md §3 has the tables).  Override one for an A/B build:
//   make -C csrc variant VOUT=../../abl/lib_x.so VF=4096 VFLAGS=-DMIMO_PRE_EW_4096=0
// (Diagnostic-only switches that change results -- MIMO_DIAG_LUT_SEQ in real.h, MIMO_DIAG_ROWS2
// in wave_fft.h, MIMO_ABLATION -- stay next to the code they alter.)
#pragma once

// ---- occupancy (trial_inst.hip profile_for)
// fp64 F <= 2048: waves / SIMD the register allocation targets.  3: 168 VGPRs, 3 teams / CU.
// 4 (with the exchange LDS halved, diagnostic) measured +3.1 %: 73 VGPRs spill
// (profiles/r06/w4/).
#ifndef MIMO_W64_2048
#define MIMO_W64_2048 3
#endif

// ---- the Bussgang gain alpha_a per antenna (trial_kernel.h array_pass)
// Formed by one wave per antenna and handed over in LDS (0: every wave forms it): config 2
// -1.0 %, CSI -1.2 %, config-5 array -2.3 % (profiles/r05/ab/ab_*_alpha1.json).
#ifndef MIMO_ALPHA1
#define MIMO_ALPHA1 1
#endif
// ... at F 4096 (fp64) too since round 6, with the cold paths out of line there: -1.4 % together
// (profiles/r06/k4096/; alone +0.8 % in round 5).
#ifndef MIMO_ALPHA1_4096
#define MIMO_ALPHA1_4096 1
#endif

// ---- pass 1 of the fp64 wave-split instances (F <= 2048) with a perfect-CSI Rayleigh channel
// (trial_kernel.h P1_*).  The array pass's register budget does not bind there: its d, r, g, h and
// the FFT temporaries are not live yet.  Config 2, 100 interleaved rounds, A/A spread 0.03 ms
// (profiles/r16/pass1_vk/ab_long.json): HOIST -0.22 ms (-0.5 %), SUMS3 -0.10 ms (-0.2 %), both
// -0.35 ms (-0.8 %); the pass-1 loop 157 -> 141 VALU per antenna-wave, registers and scratch as
// before.
// P1_HOIST: the thread id laundered once ahead of the loop instead of per antenna, so the
// counters of the two Philox calls are formed once, and thread 0's pair swap is applied to the
// finished sums once per trial, not to every antenna's words (0: per antenna, as the array pass
// must).
// P1_SUMS3: three running sums per slot, c tab, c poly and c e of real.h ln_unit_parts, assembled
// into the norm once per trial (3 FMAs per draw instead of 4; 0: every log finished per draw).
// The sum order differs, so the norm moves in its last bits: against the long-double sum 4.1
// units of the last place at most where the per-draw form has 7.3
// (tests/test_pass1_logsum_cpu.py).
#ifndef MIMO_P1_HOIST
#define MIMO_P1_HOIST 1
#endif
#ifndef MIMO_P1_SUMS3
#define MIMO_P1_SUMS3 1
#endif

// ---- the vk partials of the fp64 wave-split instances without CSI per thread in LDS (1.5 KiB
// per 256-thread team: 53,296 B of LDS, three teams per CU still): one ds_write_b64 per thread
// of the three other waves, and the antenna's alpha wave adds them per lane to its own and runs
// the one DPP tree (0: every wave reduces its own partial).  The sum order differs from the
// tree-per-wave form, so alpha moves in its last bits.  Config 2 -0.34 ms (-0.8 %), with the two
// above -0.59 ms (-1.3 %), SQ_INSTS_VALU 2.012e10 -> 1.972e10 per launch
// (profiles/r16/pass1_vk/).
#ifndef MIMO_VK_LDS
#define MIMO_VK_LDS 1
#endif

// ---- the wave that forms alpha in the fp64 wave-split instances without CSI (trial_kernel.h
// ALPHA_WAVE).  -1: wave a mod W of antenna a, so the ~47 VALU of the partial sum and the 18-FMA
// polynomial rotate over the team.  k >= 0: wave k mod W for every antenna.  Wave 0 of a team is
// the one that skips the inter-step twiddle multiply of wave_fft.h run_second (50 VALU per
// antenna fewer than waves 1..3), so 0 puts alpha on the lightest wave and 1 is the control that
// puts it on a full one.  Config 2, 100 interleaved rounds, A/A spread 0.03 ms
// (profiles/r17/balance/ab_switches.json): 0 -0.16 ms (-0.35 %), 1 +0.06 ms against -1; static
// VALU of the slowest wave per antenna 1,051 -> 999, SQ_WAIT_ANY 0.159 -> 0.149 of wave cycles
// with the series below.  The CSI instances (no VK_LDS) keep a mod W.
#ifndef MIMO_ALPHA_WAVE
#define MIMO_ALPHA_WAVE 0
#endif

// ---- the series of the Rayleigh channel draws in the fp64 wave-split instances (real.h
// ln_unit / sincos_lut DEG; every other caller -- noise, CSI, the team-FFT sizes, the probe --
// keeps the full series).  Bounds: tests/test_draw_series_cpu.py.
// P1_LN_DEG (6 | 4): log1p's last power in pass 1's weighted log sum (channel.h power_acc).  The
// t^5 and t^6 terms are below 2e-16 each where the sum of ~64 has a spacing of 1.4e-14: against
// the long-double sum 4.14 units of the last place at most with either degree.  -8 VALU per
// antenna-wave.
// BM_LN_DEG (6 | 5): the same in the array pass's radius (channel.h normals_w), under sqrt_n1's
// own 2^-47.8: per draw 1.69 units of the last place at most to t^5, 1.00 to t^6 (t^4: 1,617, so
// not there).  -4 VALU.
// BM_SIN_DEG (7 | 5): the sine's last term in normals_w's sincos_lut.  -4 VALU.
// The same run, each alone against all off: P1_LN_DEG 4 -0.30 ms (-0.7 %), BM_LN_DEG 5 -0.16 ms
// (-0.4 %), BM_SIN_DEG 5 -0.19 ms (-0.4 %); all four switches -0.77 ms (-1.7 %, 44.97 -> 44.19 ms),
// SQ_INSTS_VALU 1,175.3 -> 1,154.3 per antenna-wave, error totals and the bench's outputs equal
// (profiles/r17/balance/).
#ifndef MIMO_P1_LN_DEG
#define MIMO_P1_LN_DEG 4
#endif
#ifndef MIMO_BM_LN_DEG
#define MIMO_BM_LN_DEG 5
#endif
#ifndef MIMO_BM_SIN_DEG
#define MIMO_BM_SIN_DEG 5
#endif

// ---- the transforms' LDS and twiddle addresses of the fp64 wave-split instances without CSI held
// across the antenna loop, two 16-bit byte addresses per VGPR (wave_fft.h XAddr; three words),
// instead of re-derived from the thread id by every transform.  The words are what the transforms
// launder, in place, so the unpacked forms are not hoisted (team_fft.h run).  Every LDS byte
// address of these teams is below 34,816 and a multiple of 16 (static_assert in wave_fft.h, and
// every thread's and use site's by tests/test_xaddr_host.py).  Outputs bit for bit the parent's.
// XADDR: the LDS addresses -- the cross-wave base 16 t, the wave's row plus lane, the sub-transform's
// transposed exchange 0 read, exchange 1's padded write and read, the lane's offset in the rows of
// the stage constants; one v_and_b32 / v_lshrrev_b32 per use.  At F 1024 (two waves, stage
// twiddles instead of cot-tan constants) stage 2's base twiddles are loaded at that offset from
// a uniform base as well.  XADDR_TW, on top of it (nothing without it): the inter-step twiddle
// loads take a 32-bit per-lane byte offset (16 k t; 16 w l) and a wave-uniform base per butterfly
// / register formed on the SALU per transform, instead of 64-bit per-lane arithmetic.
// Config 2, 100 interleaved rounds, A/A spread 0.01 ms (profiles/r22/xaddr/ab_switches.json): both
// off 43.60 ms (= the parent, 43.61), XADDR alone -0.29 ms (-0.7 %), both -0.75 ms (-1.7 %, 42.86 ms
// in ab_long.json); 2mcnc -0.78 / -2.36 ms of 122.8 (-1.9 %), 2los -0.18 / -0.67 ms of 40.1 (-1.7 %).
// Static VALU per antenna of the config-2 instance: every wave 941 -> 907 -> 894, waves 1-3 add
// 50 -> 50 -> 34; SQ_INSTS_VALU 1,154.3 -> 1,095.9 per antenna-wave (-58.4, static -59.0), VGPRs
// 168, LDS 53,296 B and the loops free of scratch as before.  Time follows the count less than in
// rounds 16 / 17 (-5.1 % instructions, -1.7 % time): what went are full-rate 32-bit integer
// operations, and VALU busy fell from 0.815 to 0.785 of the SIMD.  An instance whose scratch would
// grow keeps re-deriving (trial_kernel.h xaddr_inst_ok).
#ifndef MIMO_XADDR
#define MIMO_XADDR 1
#endif
#ifndef MIMO_XADDR_TW
#define MIMO_XADDR_TW 1
#endif

// ---- Philox rounds whose words are uniform across the team on the SALU (philox.h kUni)
// Always in the fp64 wave-split instances (F <= 2048).  F 4096: with CSI only (-2.4 % on the
// paper-CSI line, +1.1 % without CSI, profiles/r06/k4096/).  F 8192: with the folded weight
// below (-1.6 % for both, profiles/r06/k8192/).
#ifndef MIMO_UNI_4096_CSI
#define MIMO_UNI_4096_CSI 1
#endif
#ifndef MIMO_UNI_8192
#define MIMO_UNI_8192 1
#endif

// ---- CSI pass 1 in polar form (Rayleigh CSI instances, fp64): -4.8 % on the CSI line
// (profiles/r05/ab/ab_2csi_polar.json).  0: two Cartesian Box-Muller draws per slot.
#ifndef MIMO_CSI_POLAR
#define MIMO_CSI_POLAR 1
#endif

// ---- the precoding weight w = 1 / ||Hhat|| / sqrt(F) folded into the channel (PRE_EW; with
// perfect CSI the loops then carry h w, WSC, and the Rayleigh draws take w in their radius,
// WSC_RAY).  Wave-split instances: -1.1 % (round 3).  F 4096: -2.8 % once the cold paths were out
// of line (round 6); F 8192: -1.3 %.  Not with CSI: +3.1 % at F 4096, the F 2048 CSI line -1.3 %
// without it (profiles/r06/k2048/ab_2csi_preew.json).
#ifndef MIMO_PRE_EW_4096
#define MIMO_PRE_EW_4096 1
#endif
#ifndef MIMO_PRE_EW_8192
#define MIMO_PRE_EW_8192 1
#endif
#ifndef MIMO_PRE_EW_CSI
#define MIMO_PRE_EW_CSI 0
#endif
#ifndef MIMO_WSC_RAY
#define MIMO_WSC_RAY 1
#endif

// ---- the cold paths (general-p Rapp, the exact-alpha fallback) out of line at F 4096 too:
// scratch 492 -> 288 B/lane, traffic 108 -> 31 KB per trial, paper -1.0 % (round 6; +1.6 % in
// round 3).  The other fp64 instances always have them out of line.
#ifndef MIMO_COLD_OUT_4096
#define MIMO_COLD_OUT_4096 1
#endif

// ---- |Hhat|^2 recomputed after the FFT (E2_RE) also with CSI: +1.7 % (F 2048) / +2.7 %
// (F 4096): the estimate stays live across both transforms (profiles/r06/k2048/ab_2csi_e2.json).
#ifndef MIMO_E2_RE_CSI
#define MIMO_E2_RE_CSI 0
#endif

// ---- F 4096: two int8 lattice levels per VGPR (SLAB8): -2.2 % in round 4; one level per word
// +3.9 % at round 6 (profiles/r06/k4096/ab_paper_s8.json).
#ifndef MIMO_SLAB8_4096
#define MIMO_SLAB8_4096 1
#endif

// ---- fp64 F 8192 (split_fft.h): two 4096-point sub-transforms on the lane halves and a
// radix-2 stage through v_permlane32_swap: -6.2 % against the 8192-point team (0: the team);
// their stages in cot-tan form: -2.4 % (profiles/r05/split/ab_5su_split.json).
#ifndef MIMO_SPLIT_FFT
#define MIMO_SPLIT_FFT 1
#endif
#ifndef MIMO_SPLIT_CT
#define MIMO_SPLIT_CT 1
#endif

// ---- team FFT (team_fft.h): the cot-tan constants of stage s + 1 loaded before stage s's
// exchange: paper +1.6 %, config-5 array +5.3 % (profiles/r06/k4096/, k8192/ab_5su_ctpf.json).
#ifndef MIMO_CT_PF
#define MIMO_CT_PF 0
#endif

// ---- envelope instances (trial_kernel.h ENV; tools/envelope_bench.py, profiles/r12/envelope/)
// fp64 F <= 2048: waves / SIMD the register allocation of the envelope instances targets.  They
// hold the PA input x across pa_block (4 P VGPRs) next to what the plain instance holds.  At 3
// (168 VGPRs, the plain instances' target) that copy spills -- scratch 144 -> 384 B / lane at
// config 2 -- and the kernel takes 1.991 ms per 1,024 trials against the plain 0.711 (+180 %); at 2
// (256 VGPRs, two 4-wave teams per CU instead of three) 0.844 ms (+20 %).  Measured at F 2048 only.
#ifndef MIMO_ENV_W64_2048
#define MIMO_ENV_W64_2048 2
#endif
// Copies of the team's LDS histogram, one per lane residue (lane mod SUBH), summed when the row is
// stored.  The samples are near-Gaussian, so most of a wave's lanes meet in the few bins around
// the mean and their ds_add_u32 to one cell queue up; SUBH copies of a cell in neighbouring banks
// split that queue.  1: the plain form, 1 KiB of LDS per team; 4: 4 KiB.  Config 2 at 2 waves / SIMD:
// 0.835 ms per 1,024 trials with 4 copies against 0.844 with 1 (-1.1 %, the spread between rounds
// is 1.3 %), both histograms together cost 0.064 ms of it; the paper geometry (F 4096) +10 % with
// 4 copies (82,544 B of LDS: one team per CU instead of two), +0.8 % with 2; at F 8192 4 copies
// do not fit the CU's LDS.  So 1.
#ifndef MIMO_ENV_SUBH
#define MIMO_ENV_SUBH 1
#endif

// ---- soft instances (trial_kernel.h SOFT; tools/soft_bench.py, profiles/r18/soft/)
// fp64 F 2048: waves / SIMD the register allocation of the soft instances targets.  Their additions
// sit in the receiver phase, outside the antenna loop, but at 3 (168 VGPRs, the plain instances'
// target) they spill more than the plain instance does -- config 2's instance: 30 -> 49 spilled
// VGPRs, scratch 144 -> 224 B / lane (profiles/r18/soft/resources.txt) -- and the kernel takes
// 0.875 ms per 1,024 trials (CNC iterations 0-4 recorded) against the plain 0.737 (+18.8 %); at 2
// (217 VGPRs, none spilled, scratch 32 B / lane; two 4-wave teams per CU instead of three) 0.839 ms
// (+14.4 %), outside the 1 % spread of either.  Measured at F 2048, and applied there only: the
// soft instances below keep the plain instances' target (F 128 and F 512 spill nothing more there;
// F 256 and F 1024 do, 12 -> 32 and 32 -> 51 VGPRs at their Rayleigh instances, unmeasured).
#ifndef MIMO_SOFT_W64_2048
#define MIMO_SOFT_W64_2048 2
#endif

// ---- coded instances (trial_kernel.h CODED; tools/coded_bench.py, profiles/r19/coded/)
// fp64 F 2048: waves / SIMD the register allocation of the coded instances targets.  Unlike the
// soft and envelope instances they keep the plain instances' 3: there config 2's instance spills
// 122 VGPRs against the plain 30 (scratch 144 -> 496 B / lane, profiles/r19/coded/resources.txt)
// and the kernel takes 0.888 ms per 1,024 trials (CNC iterations 0-4 recorded) against the plain
// 0.775 (+14.5 %); at 2 (237 VGPRs, none spilled; two 4-wave teams per CU instead of three)
// 0.929 ms (+19.9 %), medians of alternating rounds (ab_waves.json).
#ifndef MIMO_CODED_W64_2048
#define MIMO_CODED_W64_2048 MIMO_W64_2048
#endif
