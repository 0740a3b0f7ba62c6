// gdsp_corr_derive.h -- what correlate (gdsp_xsum_pair.hip) and correlateover (gdsp_intervalcorr.hip) derive on the host,
// in plain IEEE double and operation by operation, from the once-rounded figures of a pair sample: the standard
// deviations, the correlation, the slope and the intercept (include/genodsp_hip.h spells them at gdsp_genome_correlation).
#pragma once

#include <float.h>
#include <math.h>
#include "gdsp_common.h"

// fl(a * b), never contracted into what follows
static inline double gdsp_corr_mul (double a, double b) { volatile double p = a * b;  return p; }

// out[GDSP_CORR_FIGURES] of a sample that is not empty, with MEANX, MEANY, VARX, VARY and COV in place and NaN in
// CORRELATION, SLOPE and INTERCEPT: SDX and SDY, and those three where they are defined
static inline void gdsp_corr_derive (double* out)
	{
	const double varx = out[GDSP_CORR_VARX], vary = out[GDSP_CORR_VARY], cov = out[GDSP_CORR_COV];
	const double sdx  = out[GDSP_CORR_SDX] = sqrt (varx);
	const double sdy  = out[GDSP_CORR_SDY] = sqrt (vary);
	const bool xok = (varx > 0) && (varx <= DBL_MAX), yok = (vary > 0) && (vary <= DBL_MAX), cok = !isnan (cov);
	if (xok && yok && cok)
		{
		int ex, ey;
		const double mx = frexp (sdx, &ex), my = frexp (sdy, &ey);
		double r = ldexp (cov, -(ex + ey)) / gdsp_corr_mul (mx, my);
		if (r >  1.0) r =  1.0;
		if (r < -1.0) r = -1.0;
		out[GDSP_CORR_CORRELATION] = r;
		}
	if (xok && cok)
		{
		const double slope = out[GDSP_CORR_SLOPE] = cov / varx;
		out[GDSP_CORR_INTERCEPT] = out[GDSP_CORR_MEANY] - gdsp_corr_mul (slope, out[GDSP_CORR_MEANX]);
		}
	}
