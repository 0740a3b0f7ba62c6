/* ops_fused.c -- operator chains that run as one kernel.
 *
 * The reference runs a maximal run of per-chromosome operators back to back on each
 * chromosome "for cache performance" (genodsp.c:895-921).  On the GPU the analogue is not to
 * let the intermediate signal leave the chip at all: for the chains the device library fuses
 * (`= smooth = localmax|localmin`, `= dilate = erode [= binarize]`) the driver makes one
 * call, with results bit-identical to the separate operators (tests/test_hip_parity.py). */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_window_sum)     dspprototypes(op_smooth)        dspprototypes(op_cumulative_sum)
dspprototypes(op_percentile)     dspprototypes(op_add)           dspprototypes(op_subtract)
dspprototypes(op_add_constant)   dspprototypes(op_invert)        dspprototypes(op_multiply)
dspprototypes(op_divide)         dspprototypes(op_absolute_value) dspprototypes(op_clip)
dspprototypes(op_erase)          dspprototypes(op_binarize)      dspprototypes(op_local_minima)
dspprototypes(op_local_maxima)   dspprototypes(op_best_local_min) dspprototypes(op_best_local_max)
dspprototypes(op_close)          dspprototypes(op_open)          dspprototypes(op_dilate)
dspprototypes(op_erode)          dspprototypes(op_input)         dspprototypes(op_output)
dspprototypes(op_show_variables) dspprototypes(op_mask)          dspprototypes(op_mask_not)
dspprototypes(op_or)             dspprototypes(op_and)           dspprototypes(op_min_with)
dspprototypes(op_max_with)       dspprototypes(op_map)           dspprototypes(op_min_in_interval)
dspprototypes(op_max_in_interval) dspprototypes(op_clump)        dspprototypes(op_skimp)

/* ---- what the driver knows about the reference's operators (optraits, host_services.h); slidingsum has nothing to say */
static int smooth_reach (dspop* op, u32* left, u32* right)             /* sum.c:647-663: taps -h..+h */
	{ *left = *right = (op_smooth_window (op) - 1) / 2;  return true; }
static int local_reach (dspop* op, u32* left, u32* right)              /* minmax.c:1195-1216 */
	{ u32 N;  int wantMax;  valtype fill;  op_local_describe (op, &N, &wantMax, &fill);  *left = *right = (N - 1) / 2;  return true; }
static int best_reach (dspop* op, u32* left, u32* right) { return reach_centred (op_best_window (op), left, right); }
static int morph_reach (dspop* op, u32* left, u32* right) { op_morph_reach (op, left, right);  return (*left != u32Max); }

/* one launch per device; GDSP_EINVAL from the extrema and the morphology: no tiled kernel takes this window */
static int smooth_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{ return gdsp_smooth_batch (items, n, op_smooth_window (op), firMode, st); }
static int local_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{ u32 N;  int wantMax;  valtype fill;  op_local_describe (op, &N, &wantMax, &fill);  return gdsp_local_extrema_batch (items, n, N, wantMax, fill, st); }
static int best_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{ return gdsp_best_extrema_batch (items, n, op_best_window (op), op->funcApply == op_best_local_max_apply, st); }
static int morph_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{
	u32 l, r;  valtype T, one, zero;
	op_morph_describe (op, &l, &r, &T, &one, &zero);
	return (op->funcApply == op_dilate_apply)? gdsp_dilate_batch (items, n, l, r, T, one, zero, st)
	                                         : gdsp_erode_batch  (items, n, l, r, T, one, zero, st);
	}
static int binarize_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{ valtype T, one, zero;  int ties;  op_binarize_describe (op, &T, &ties, &one, &zero);  return gdsp_binarize_batch (items, n, T, ties, one, zero, st); }
static int limits_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{
	int haveMin, haveMax, keepInside;  valtype lo, hi, zero;
	op_limits_describe (op, &haveMin, &lo, &haveMax, &hi, &keepInside, &zero);
	return (op->funcApply == op_clip_apply)? gdsp_clip_batch  (items, n, haveMin, lo, haveMax, hi, st)
	                                       : gdsp_erase_batch (items, n, haveMin, lo, haveMax, hi, keepInside, zero, st);
	}
static int add_constant_batch (dspop* op, const gdsp_batch_item* items, int n, void* st)
	{ return gdsp_add_constant_batch (items, n, op_add_constant_value (op), st); }
static int abs_batch (dspop* op, const gdsp_batch_item* items, int n, void* st) { return gdsp_abs_batch (items, n, st); }

const optraits coreTraits[] =
	{ /* apply                    inPlace onParts reach         batch               work */
	{ op_window_sum_apply,        true,  false, NULL,         NULL,               NULL },
	{ op_smooth_apply,            false, false, smooth_reach, smooth_batch,       NULL },
	{ op_cumulative_sum_apply,    true,  false, NULL,         NULL,               NULL },
	{ op_clump_apply,             true,  false, NULL,         NULL,               NULL },
	{ op_skimp_apply,             true,  false, NULL,         NULL,               NULL },
	{ op_percentile_apply,        true,  true,  NULL,         NULL,               NULL },   /* (but see percentile = binarize) */
	{ op_add_apply,               true,  false, NULL,         NULL,               NULL },
	{ op_subtract_apply,          true,  false, NULL,         NULL,               NULL },
	{ op_add_constant_apply,      true,  false, reach_none,   add_constant_batch, NULL },
	{ op_invert_apply,            true,  true,  NULL,         NULL,               NULL },
	{ op_multiply_apply,          true,  false, NULL,         NULL,               NULL },
	{ op_divide_apply,            true,  false, NULL,         NULL,               NULL },
	{ op_absolute_value_apply,    true,  false, reach_none,   abs_batch,          NULL },
	{ op_mask_apply,              true,  false, NULL,         NULL,               NULL },
	{ op_mask_not_apply,          true,  false, NULL,         NULL,               NULL },
	{ op_clip_apply,              true,  false, reach_none,   limits_batch,       NULL },
	{ op_erase_apply,             true,  false, reach_none,   limits_batch,       NULL },
	{ op_binarize_apply,          true,  false, reach_none,   binarize_batch,     NULL },
	{ op_or_apply,                true,  false, NULL,         NULL,               NULL },
	{ op_and_apply,               true,  false, NULL,         NULL,               NULL },
	{ op_max_in_interval_apply,   true,  false, NULL,         NULL,               NULL },
	{ op_min_in_interval_apply,   true,  false, NULL,         NULL,               NULL },
	{ op_local_minima_apply,      false, false, local_reach,  local_batch,        NULL },
	{ op_local_maxima_apply,      false, false, local_reach,  local_batch,        NULL },
	{ op_best_local_min_apply,    false, false, best_reach,   best_batch,         NULL },
	{ op_best_local_max_apply,    false, false, best_reach,   best_batch,         NULL },
	{ op_min_with_apply,          true,  false, NULL,         NULL,               NULL },
	{ op_max_with_apply,          true,  false, NULL,         NULL,               NULL },
	{ op_close_apply,             false, false, morph_reach,  NULL,               NULL },
	{ op_open_apply,              false, false, morph_reach,  NULL,               NULL },
	{ op_dilate_apply,            false, false, morph_reach,  morph_batch,        NULL },
	{ op_erode_apply,             false, false, morph_reach,  morph_batch,        NULL },
	{ op_map_apply,               true,  false, reach_none,   NULL,               NULL },
	{ op_input_apply,             true,  false, NULL,         NULL,               NULL },
	{ op_output_apply,            true,  false, NULL,         NULL,               NULL },
	{ op_show_variables_apply,    true,  true,  NULL,         NULL,               NULL } };
const int coreTraitsLen = (int) (sizeof(coreTraits)/sizeof(coreTraits[0]));

int op_reach (dspop* op, u32* left, u32* right)
	{
	const optraits* t = traits_of (op);
	*left = *right = 0;
	return (t != NULL) && (t->reach != NULL) && (*t->reach) (op, left, right);
	}

int try_fused_apply (dspop* op, dspop* stopOp, spec* s)
	{
	dspop* next = op->next;
	if ((next == NULL) || (next == stopOp)) return 0;

	if ((op->funcApply == op_smooth_apply)
	 && ((next->funcApply == op_local_maxima_apply) || (next->funcApply == op_local_minima_apply)))
		{
		u32 N;  int wantMax;  valtype fill;
		op_local_describe (next, &N, &wantMax, &fill);
		if (!gdsp_smooth_local_extrema_fusable (op_smooth_window (op), N)) return 0;
		check_gdsp (gdsp_smooth_local_extrema (s->valVector, partner_vector (s->chrom), s->length,
		                                       op_smooth_window (op), firMode, N, wantMax, fill, op_stream ()), op->name);
		flip_vector (s->chrom);
		return 2;
		}

	if ((op->funcApply == op_dilate_apply) && (next->funcApply == op_erode_apply))
		{
		u32 dl, dr, el, er;  valtype dT, dOne, dZero, eT, eOne, eZero;
		valtype bT = 0, bOne = 1, bZero = 0;  int bTies = false, withBinarize = false;
		op_morph_describe (op,   &dl, &dr, &dT, &dOne, &dZero);
		op_morph_describe (next, &el, &er, &eT, &eOne, &eZero);
		dspop* third = next->next;
		if ((third != NULL) && (third != stopOp) && (third->funcApply == op_binarize_apply))
			{ op_binarize_describe (third, &bT, &bTies, &bOne, &bZero);  withBinarize = true; }
		int rc = gdsp_dilate_erode (s->valVector, partner_vector (s->chrom), s->length,
		                            dl, dr, dT, dOne, dZero, el, er, eT, eOne, eZero,
		                            withBinarize, bT, bTies, bOne, bZero, op_stream ());
		if (rc == GDSP_EINVAL) return 0;          /* reach too long for one tile: run them separately */
		check_gdsp (rc, op->name);
		flip_vector (s->chrom);
		return withBinarize? 3 : 2;
		}
	return 0;
	}

/* ---- one launch per operator per device (gdsp_*_batch): the chromosome loop of genodsp.c:909-921 turned inside out.
 * Chromosomes are independent for every per-chromosome operator, so "every operator of the run on chromosome 1, then
 * on chromosome 2, ..." and "operator 1 on every chromosome, then operator 2, ..." give the same signal; the second
 * order lets one grid cover all the vectors a device owns (no ramp and drain between 24 short kernels). */
int op_batchable (dspop* op)
	{
	const optraits* t = traits_of (op);
	return (t != NULL) && (t->batch != NULL);
	}

/* the chains the device library fuses, and a smooth that feeds an extremum (which is not evaluated as hann, fused or not:
 * as op_smooth_apply / try_fused_apply); returns how many operators *rc speaks for, 0 when op heads no such chain */
static int chain_batch (dspop* op, dspop* next, dspop* stopOp, const gdsp_batch_item* items, int nunits, int allowFusion, void* st, int* rc)
	{
	opfunc_apply f = op->funcApply;
	if (next == NULL) return 0;
	if ((f == op_smooth_apply) && ((next->funcApply == op_local_maxima_apply) || (next->funcApply == op_local_minima_apply)))
		{
		int mode = (firMode == GDSP_FIR_HANN)? GDSP_FIR_FMA : firMode;
		u32 N;  int wantMax;  valtype fill;
		op_local_describe (next, &N, &wantMax, &fill);
		if (allowFusion && gdsp_smooth_local_extrema_fusable (op_smooth_window (op), N))
			{ *rc = gdsp_smooth_local_extrema_batch (items, nunits, op_smooth_window (op), mode, N, wantMax, fill, st);  return 2; }
		*rc = gdsp_smooth_batch (items, nunits, op_smooth_window (op), mode, st);
		return 1;
		}
	if (allowFusion && (f == op_dilate_apply) && (next->funcApply == op_erode_apply))
		{
		u32 l, r, el, er;  valtype T, one, zero, eT, eOne, eZero, bT = 0, bOne = 1, bZero = 0;  int bTies = false, withBinarize = false;
		op_morph_describe (op,   &l,  &r,  &T,  &one,  &zero);
		op_morph_describe (next, &el, &er, &eT, &eOne, &eZero);
		if (!gdsp_dilate_erode_fusable (l, r, el, er)) return 0;     /* (a property of the reaches alone: every device decides alike) */
		dspop* third = next->next;
		if ((third != NULL) && (third != stopOp) && (third->funcApply == op_binarize_apply))
			{ op_binarize_describe (third, &bT, &bTies, &bOne, &bZero);  withBinarize = true; }
		*rc = gdsp_dilate_erode_batch (items, nunits, l, r, T, one, zero, el, er, eT, eOne, eZero,
		                               withBinarize, bT, bTies, bOne, bZero, st);
		return withBinarize? 3 : 2;
		}
	return 0;
	}

/* apply op -- and the operators fused behind it -- to units[0..nunits), all of them on the current device;
 * returns how many operators were consumed (>= 1; op must be batchable) */
int batch_apply_on_device (dspop* op, dspop* stopOp, spec** units, int nunits, int allowFusion)
	{
	const optraits* t = traits_of (op);
	opfunc_apply f = op->funcApply;
	gdsp_batch_item* items = (gdsp_batch_item*) calloc (nunits? nunits : 1, sizeof(gdsp_batch_item));
	if (items == NULL) { fprintf (stderr, "out of memory\n");  exit (EXIT_FAILURE); }
	/* (the in-place operators never ask for a partner: a pipeline of them alone runs without the partners' arena) */
	for (int i=0 ; i<nunits ; i++)
		{
		items[i].n = units[i]->length;
		if (t->inPlace) { items[i].d_in = NULL;                 items[i].d_out = units[i]->valVector; }
		else            { items[i].d_in = units[i]->valVector;  items[i].d_out = partner_of (units[i]); }
		}
	void* st = op_stream ();
	int   rc = GDSP_OK;
	int   consumed = chain_batch (op, (op->next == stopOp)? NULL : op->next, stopOp, items, nunits, allowFusion, st, &rc);
	if (consumed == 0)
		{
		consumed = 1;
		rc = (*t->batch) (op, items, nunits, st);
		int tiledOnly = (f == op_local_maxima_apply) || (f == op_local_minima_apply) || (f == op_best_local_max_apply)
		             || (f == op_best_local_min_apply) || (f == op_dilate_apply) || (f == op_erode_apply);
		if (tiledOnly && (rc == GDSP_EINVAL)) goto one_by_one;     /* neighbourhood, window or reach beyond one LDS tile */
		}
	free (items);
	check_gdsp (rc, op->name);
	if (!t->inPlace) { for (int i=0 ; i<nunits ; i++) flip_spec (units[i]); }
	return consumed;

	/* no tiled kernel takes this window: the operator's own apply, vector by vector, which goes on to its
	 * whole-vector route (gdsp_*_any); nothing has been flipped, whatever a refused batch call wrote went to partners */
one_by_one:
	free (items);
	for (int i=0 ; i<nunits ; i++) apply_to_unit (op, units[i]);
	return 1;
	}
