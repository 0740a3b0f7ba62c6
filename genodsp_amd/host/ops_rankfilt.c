/* ops_rankfilt.c -- slidingpercentile and median (device shims).  Not operators of the reference: a windowed order
 * statistic, the robust smoother the reference has no counterpart for.  Window, centring and edge rule are bestmax's
 * (ops_minmax.c, minmax.c:1527-1603 / :1616-1640 in the reference); P is read like percentile's single value and
 * converted by the same to_thousandths, but a P outside 0..100 (or one that is not a number) is refused here, where
 * percentile clamps it: a running percentile above 100 is a typing error, not a request for the maximum.
 * The definition is at gdsp_sliding_percentile (include/genodsp_hip.h).
 *
 * The driver finds these operators through opgroup_rankfilt, at the end of this file (host_services.h); every call into the
 * device library for them stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_sliding_percentile)  dspprototypes(op_sliding_median)

typedef struct dspop_rankfilt { dspop common;  u32 windowSize;  u32 pThousandths; } dspop_rankfilt;

static dspop* rankfilt_parse (char* name, int argc, char** argv, int isMedian)
	{
	dspop_rankfilt* op = (dspop_rankfilt*) new_op (name, sizeof(dspop_rankfilt), false);
	int havePercentile = isMedian;
	op->windowSize   = (u32) get_named_global ("windowSize", 100);
	op->pThousandths = 50000;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (is_opt3 (arg, "window", "W")) { op->windowSize = window_arg (name, arg, argVal, "window size");  continue; }
		if (strcmp (arg, "--debug") == 0) continue;
		if (!isMedian && !havePercentile && (strcmp_prefix (arg, "--") != 0))
			{
			valtype pct;
			if (!try_string_to_valtype (arg, &pct))
				chastise ("[%s] \"%s\" is not a percentile\n", name, arg);
			if (!((pct >= 0.0) && (pct <= 100.0)))
				chastise ("[%s] percentile must be between 0 and 100 (\"%s\")\n", name, arg);
			op->pThousandths = to_thousandths (pct);
			havePercentile = true;
			continue;
			}
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (!havePercentile) chastise ("[%s] no percentile was provided\n", name);
	if (op->windowSize > GDSP_SLIDING_PERCENTILE_MAX_WINDOW)
		chastise ("[%s] window size %u is above the largest this operator supports (%d)\n",
		          name, op->windowSize, GDSP_SLIDING_PERCENTILE_MAX_WINDOW);
	return (dspop*) op;
	}

static void rankfilt_usage (char* name, FILE* f, char* indent, int isMedian)
	{
	if (indent == NULL) indent = "";
	if (isMedian) fprintf (f, "%sReplace every base by the median over the window centred on it.\n", indent);
	else          fprintf (f, "%sReplace every base by the given percentile over the window centred on it.\n", indent);
	fprintf (f, "%sBases beyond the ends of the chromosome are not considered. Not in genodsp.\n\n", indent);
	if (isMedian) fprintf (f, "%susage: %s [options]\n", indent, name);
	else          fprintf (f, "%susage: %s <percentile> [options]\n", indent, name);
	if (!isMedian) fprintf (f, "%s  <percentile>             0 to 100, in steps of 0.001 (a value outside is refused,\n", indent);
	if (!isMedian) fprintf (f, "%s                           where percentile would clamp it)\n", indent);
	fprintf (f, "%s  --window=<length>        (W=) window size (default: global window, else 100; at most %d)\n",
	         indent, GDSP_SLIDING_PERCENTILE_MAX_WINDOW);
	}

static void rankfilt_apply (dspop* _op, char* vName, u32 vLen, valtype* v)
	{
	dspop_rankfilt* op = (dspop_rankfilt*) _op;
	check_gdsp (gdsp_sliding_percentile (v, partner_vector (vName), vLen, op->windowSize, op->pThousandths, op_stream ()),
	            _op->name);
	flip_vector (vName);
	}

/* the driver: bestmax's window, and one launch per device (windows above the maximum were refused at parse time) */
static int rankfilt_reach (dspop* op, u32* left, u32* right) { return reach_centred (((dspop_rankfilt*) op)->windowSize, left, right); }

static int rankfilt_batch (dspop* _op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	dspop_rankfilt* op = (dspop_rankfilt*) _op;
	return gdsp_sliding_percentile_batch (items, nitems, op->windowSize, op->pThousandths, stream);
	}

OP_SHORT (op_sliding_percentile, "percentile over a sliding window (not in genodsp)")
void   op_sliding_percentile_usage (char* name, FILE* f, char* indent) { rankfilt_usage (name, f, indent, false); }
dspop* op_sliding_percentile_parse (char* name, int argc, char** argv) { return rankfilt_parse (name, argc, argv, false); }
void   op_sliding_percentile_free  (dspop* op) { free (op); }
void   op_sliding_percentile_apply (dspop* op, char* vName, u32 vLen, valtype* v) { rankfilt_apply (op, vName, vLen, v); }

OP_SHORT (op_sliding_median, "median over a sliding window (not in genodsp)")
void   op_sliding_median_usage (char* name, FILE* f, char* indent) { rankfilt_usage (name, f, indent, true); }
dspop* op_sliding_median_parse (char* name, int argc, char** argv) { return rankfilt_parse (name, argc, argv, true); }
void   op_sliding_median_free  (dspop* op) { free (op); }
void   op_sliding_median_apply (dspop* op, char* vName, u32 vLen, valtype* v) { rankfilt_apply (op, vName, vLen, v); }

static const dspinfo rankfiltRows[] =
	{ dspinforecord("slidingpercentile", op_sliding_percentile), dspinfoalias ("sliding_percentile"),
	  dspinforecord("median"        , op_sliding_median) , dspinfoalias ("slidingmedian")  , dspinfoalias ("sliding_median") };
static const optraits rankfiltTraits[] =
	{ { op_sliding_percentile_apply, false, false, rankfilt_reach, rankfilt_batch, NULL },
	  { op_sliding_median_apply,     false, false, rankfilt_reach, rankfilt_batch, NULL } };
const opgroup opgroup_rankfilt = OPGROUP (rankfiltRows, rankfiltTraits, NULL);
