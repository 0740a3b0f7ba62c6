/* ops_localmad.c -- localmad and hampel (device shims).  Not operators of the reference: every base against the median and
 * the median absolute deviation (MAD) of the window centred on it -- the robust counterpart of localstats, whose mean and
 * stddev are dragged by the very towers one wants to score -- and the classic filter built on the pair, Hampel's, which
 * replaces a base by its window's median where it lies more than t scaled MADs from it.  Window, centring and edge rule
 * are slidingpercentile's (ops_rankfilt.c; bestmax's, minmax.c:1527-1603 / :1616-1640 in the reference).
 * The definition is at gdsp_localmad (include/genodsp_hip.h).  The two operators differ in their default --as only.
 *
 * The driver finds these operators through opgroup_localmad, at the end of this file (host_services.h); every call into the
 * device library for them stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_localmad)  dspprototypes(op_hampel)

typedef struct dspop_localmad
	{
	dspop   common;
	u32     windowSize;
	int     what;
	valtype scale;
	char*   thresholdVarName;  valtype threshold;
	int     haveMinMad;  char* minMadVarName;  valtype minMad;
	} dspop_localmad;

static const struct { const char* name;  int what; } figures[] =
	{ { "zscore", GDSP_LOCALMAD_ZSCORE }, { "median", GDSP_LOCALMAD_MEDIAN }, { "mad", GDSP_LOCALMAD_MAD },
	  { "difference", GDSP_LOCALMAD_DIFFERENCE }, { "clean", GDSP_LOCALMAD_CLEAN }, { "outlier", GDSP_LOCALMAD_OUTLIER } };

static void localmad_usage (char* name, FILE* f, char* indent, int isHampel)
	{
	if (indent == NULL) indent = "";
	if (isHampel)
		{
		fprintf (f, "%sThe Hampel filter: replace every base that lies more than <t> scaled MADs from the median\n", indent);
		fprintf (f, "%sof the window centred on it by that median, and leave every other base as it is.\n", indent);
		}
	else
		fprintf (f, "%sReplace every base by its value relative to the median and the MAD of the window centred on it.\n", indent);
	fprintf (f, "%sThe window is slidingpercentile's, cut off at the chromosome ends, with m bases in it, and\n", indent);
	fprintf (f, "%smedian is the value of rank m/2 (from 0; the upper median for even m), as `median` writes it.\n", indent);
	fprintf (f, "%sMAD = the value of the same rank among |value - median| over the window;\n", indent);
	fprintf (f, "%ssigma = <c> max(MAD, minmad); difference = value - median (0 where they are equal); a base is\n", indent);
	fprintf (f, "%san outlier where |difference| > <t> sigma. Every step is rounded once, so every figure is\n", indent);
	fprintf (f, "%sdefined bit for bit. With sigma = 0 every base that differs from its median is an outlier\n", indent);
	fprintf (f, "%s(--minmad tempers that). Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [options]\n", indent, name);
	fprintf (f, "%s  --window=<length>        (W=) window size (default: global window, else 100; at most %d);\n",
	         indent, GDSP_LOCALMAD_MAX_WINDOW);
	fprintf (f, "%s                           (W-1)/2 bases to the left, the rest to the right\n", indent);
	fprintf (f, "%s  --as=zscore              write difference / sigma, 0 where sigma is 0: the robust z-score\n", indent);
	if (!isHampel) fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --as=median              write the window's median: the robust local background\n", indent);
	fprintf (f, "%s  --as=mad                 write max(MAD, minmad)\n", indent);
	fprintf (f, "%s  --as=difference          write value - median\n", indent);
	fprintf (f, "%s  --as=clean               write the median where the base is an outlier, else the value itself\n", indent);
	if (isHampel) fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --as=outlier             write 1 where the base is an outlier, else 0\n", indent);
	fprintf (f, "%s  --scale=<c>              what the MAD is multiplied by (default: 1.4826, which makes sigma\n", indent);
	fprintf (f, "%s                           estimate the standard deviation of normally distributed values)\n", indent);
	fprintf (f, "%s  --threshold=<t|variable> how many sigmas make an outlier (default: 3)\n", indent);
	fprintf (f, "%s  --minmad=<value|variable> use max(MAD, this) as the MAD (as in: = stats = %s --minmad=stddev)\n", indent, name);
	}

static dspop* localmad_parse (char* name, int argc, char** argv, int isHampel)
	{
	dspop_localmad* op = (dspop_localmad*) new_op (name, sizeof(dspop_localmad), false);
	op->windowSize = (u32) get_named_global ("windowSize", 100);
	op->what       = isHampel? GDSP_LOCALMAD_CLEAN : GDSP_LOCALMAD_ZSCORE;
	op->scale      = 1.4826;
	op->threshold  = 3.0;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (is_opt3 (arg, "window", "W")) { op->windowSize = window_arg (name, arg, argVal, "window size");  continue; }
		if (strcmp_prefix (arg, "--as=") == 0)
			{
			size_t k = 0;
			while ((k < sizeof(figures)/sizeof(figures[0])) && (strcmp (argVal, figures[k].name) != 0)) k++;
			if (k == sizeof(figures)/sizeof(figures[0]))
				chastise ("[%s] --as must be zscore, median, mad, difference, clean or outlier (\"%s\")\n", name, arg);
			op->what = figures[k].what;
			continue;
			}
		if (strcmp_prefix (arg, "--scale=") == 0)
			{
			if (!try_string_to_valtype (argVal, &op->scale) || !(op->scale > 0.0) || isinf (op->scale))
				chastise ("[%s] --scale must be a finite positive number (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--threshold=") == 0)
			{
			level_arg (name, arg, argVal, &op->threshold, &op->thresholdVarName);
			if ((op->thresholdVarName == NULL) && (op->threshold < 0.0))
				chastise ("[%s] --threshold can't be negative (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--minmad=") == 0)
			{
			level_arg (name, arg, argVal, &op->minMad, &op->minMadVarName);
			if ((op->minMadVarName == NULL) && (op->minMad < 0.0))
				chastise ("[%s] --minmad can't be negative (\"%s\")\n", name, arg);
			op->haveMinMad = true;
			continue;
			}
		if (strcmp (arg, "--debug") == 0) continue;
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->windowSize > GDSP_LOCALMAD_MAX_WINDOW)
		chastise ("[%s] window size %u is above the largest this operator supports (%d)\n",
		          name, op->windowSize, GDSP_LOCALMAD_MAX_WINDOW);
	return (dspop*) op;
	}

static void localmad_free (dspop* _op)
	{
	dspop_localmad* op = (dspop_localmad*) _op;
	if (op->thresholdVarName != NULL) free (op->thresholdVarName);
	if (op->minMadVarName != NULL) free (op->minMadVarName);
	free (op);
	}

/* the variables are fetched when the operator first runs: by then `stats` or `percentile` has set them (a variable that
 * turns out negative or NaN is refused by the library, in its own words) */
static void resolve_levels (dspop_localmad* op)
	{
	resolve_variable (&op->common, &op->thresholdVarName, &op->threshold, "threshold");
	resolve_variable (&op->common, &op->minMadVarName, &op->minMad, "smallest MAD");
	}

static void localmad_apply (dspop* _op, char* vName, u32 vLen, valtype* v)
	{
	dspop_localmad* op = (dspop_localmad*) _op;
	resolve_levels (op);
	check_gdsp (gdsp_localmad (v, partner_vector (vName), vLen, op->windowSize, op->what, op->scale, op->threshold,
	                           op->haveMinMad, op->minMad, op_stream ()), _op->name);
	flip_vector (vName);
	}

/* the driver: bestmax's window -- one window's reach, not two: the deviations are taken inside the median's own window --
 * and one launch per device (windows above the maximum were refused at parse time) */
static int localmad_reach (dspop* op, u32* left, u32* right) { return reach_centred (((dspop_localmad*) op)->windowSize, left, right); }

static int localmad_batch (dspop* _op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	dspop_localmad* op = (dspop_localmad*) _op;
	resolve_levels (op);
	return gdsp_localmad_batch (items, nitems, op->windowSize, op->what, op->scale, op->threshold,
	                            op->haveMinMad, op->minMad, stream);
	}

OP_SHORT (op_localmad, "each base against the median and MAD of the window around it (not in genodsp)")
void   op_localmad_usage (char* name, FILE* f, char* indent) { localmad_usage (name, f, indent, false); }
dspop* op_localmad_parse (char* name, int argc, char** argv) { return localmad_parse (name, argc, argv, false); }
void   op_localmad_free  (dspop* op) { localmad_free (op); }
void   op_localmad_apply (dspop* op, char* vName, u32 vLen, valtype* v) { localmad_apply (op, vName, vLen, v); }

OP_SHORT (op_hampel, "Hampel filter: outliers of the window's median and MAD replaced by the median (not in genodsp)")
void   op_hampel_usage (char* name, FILE* f, char* indent) { localmad_usage (name, f, indent, true); }
dspop* op_hampel_parse (char* name, int argc, char** argv) { return localmad_parse (name, argc, argv, true); }
void   op_hampel_free  (dspop* op) { localmad_free (op); }
void   op_hampel_apply (dspop* op, char* vName, u32 vLen, valtype* v) { localmad_apply (op, vName, vLen, v); }

static const dspinfo localmadRows[] =
	{ dspinforecord("localmad", op_localmad), dspinfoalias ("local_mad"), dspinfoalias ("robustzscore"), dspinfoalias ("localrobust"),
	  dspinforecord("hampel"  , op_hampel)  , dspinfoalias ("hampelfilter"), dspinfoalias ("despike") };
static const optraits localmadTraits[] =
	{ { op_localmad_apply, false, false, localmad_reach, localmad_batch, NULL },
	  { op_hampel_apply,   false, false, localmad_reach, localmad_batch, NULL } };
const opgroup opgroup_localmad = OPGROUP (localmadRows, localmadTraits, NULL);
