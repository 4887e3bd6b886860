/* psa_plain_rk4.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * One plain classic RK4 of every sweep model (psa_plain_rk4.inc.h), instantiated per precision:
 *     psa_plain_rk4_ld    long double (x87 extended, eps 1.1e-19): the yardstick of the long runs, where the NumPy
 *                         longdouble statement (tests/truth_ld.py, 0.5 ms per step) cannot go
 *     psa_plain_rk4_f64   double: a plain float64 twin from the same text
 *     psa_plain_rk4_f32   float: the state and every operation in float32, the phase formed and reduced in float64 before
 *                         cosf / sinf; the state update plain, Kahan-compensated, or base + offset (the compensated twins)
 * Built with -ffp-contract=off: no operation is fused. */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if LDBL_MANT_DIG < 64
#error "long double has fewer than 64 mantissa bits here: the yardstick needs x87 extended precision"
#endif
#if !defined(FLT_EVAL_METHOD) || FLT_EVAL_METHOD != 0
#error "FLT_EVAL_METHOD != 0: float and double expressions would be evaluated in a wider type, and the twins would not be float32 / float64"
#endif

#define PR_MAX_WAVES 34                 /* two pumps and 16 pairs */
#define PR_MAX_LINES 16                 /* the comb model's lines */
#define PR_FOLD_EVERY 16
#define PR_TWO_PI 6.283185307179586476925286766559

enum { PR_MODEL_PAIRS = 0, PR_MODEL_SINGLE_PUMP = 1, PR_MODEL_COMB = 2 };
enum { PR_UPDATE_PLAIN = 0, PR_UPDATE_KAHAN = 1, PR_UPDATE_BASE_OFFSET = 2, PR_UPDATE_BASE_OFFSET_NO_RESIDUE = 3 };

#define T long double
#define PH long double
#define SFX _ld
#define COS_T cosl
#define SIN_T sinl
#include "psa_plain_rk4.inc.h"
#undef T
#undef PH
#undef SFX
#undef COS_T
#undef SIN_T

#define T double
#define PH double
#define SFX _f64
#define COS_T cos
#define SIN_T sin
#include "psa_plain_rk4.inc.h"
#undef T
#undef PH
#undef SFX
#undef COS_T
#undef SIN_T

#define T float
#define PH double
#define SFX _f32
#define COS_T cosf
#define SIN_T sinf
#define REDUCE_PHASE
#include "psa_plain_rk4.inc.h"
