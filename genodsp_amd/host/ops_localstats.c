/* ops_localstats.c -- localstats (device shim).  Not an operator of the reference: every base against the mean and the
 * variance of the window centred on it -- the local lambda of MACS, fold enrichment over a local mean, a local z-score.
 * Window, centring and edge rule are slidingsum's (ops_sum.c, sum.c:436-455 in the reference).
 * The definition is at gdsp_localstats (include/genodsp_hip.h).
 *
 * The driver finds this operator through opgroup_localstats, at the end of this file (host_services.h); every call into the
 * device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_localstats)

typedef struct dspop_localstats
	{
	dspop   common;
	u32     windowSize;
	int     what;
	int     haveFloor;  char* floorVarName;  valtype floor;
	int     haveMinSd;  char* minSdVarName;  valtype minSd;
	} dspop_localstats;

static const struct { const char* name;  int what; } figures[] =
	{ { "zscore", GDSP_LOCALSTATS_ZSCORE }, { "mean", GDSP_LOCALSTATS_MEAN }, { "variance", GDSP_LOCALSTATS_VARIANCE },
	  { "stddev", GDSP_LOCALSTATS_STDDEV }, { "difference", GDSP_LOCALSTATS_DIFFERENCE }, { "ratio", GDSP_LOCALSTATS_RATIO } };

OP_SHORT (op_localstats, "each base against the mean and variance of the window around it (not in genodsp)")

void op_localstats_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sReplace every base by its value relative to the window centred on it. The window is\n", indent);
	fprintf (f, "%sslidingsum's, cut off at the chromosome ends, and m is the number of bases in it.\n", indent);
	fprintf (f, "%sWith S1 the sum of the values and S2 the sum of their squares over the window:\n", indent);
	fprintf (f, "%smean = S1/m, variance = (m S2 - S1 S1) / (m m) (the population variance; 0 where that\n", indent);
	fprintf (f, "%sis not positive), stddev = sqrt(variance). Every step is rounded once; for read depth\n", indent);
	fprintf (f, "%sthe sums are exact and so is every figure. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [options]\n", indent, name);
	fprintf (f, "%s  --window=<length>        (W=) window size (default: global window, else 100; at most %d);\n",
	         indent, GDSP_LOCALSTATS_MAX_WINDOW);
	fprintf (f, "%s                           (W-1)/2 bases to the right, the rest to the left\n", indent);
	fprintf (f, "%s  --as=zscore              write (value - mean) / stddev, 0 where stddev is 0\n", indent);
	fprintf (f, "%s                           (this is the default)\n", indent);
	fprintf (f, "%s  --as=mean                write the window's mean: the local background\n", indent);
	fprintf (f, "%s  --as=variance            write the window's variance\n", indent);
	fprintf (f, "%s  --as=stddev              write the window's standard deviation\n", indent);
	fprintf (f, "%s  --as=difference          write value - mean\n", indent);
	fprintf (f, "%s  --as=ratio               write value / mean, 0 where the mean is 0\n", indent);
	fprintf (f, "%s  --floor=<value|variable> use max(mean, this) as the mean of --as=mean, difference and\n", indent);
	fprintf (f, "%s                           ratio (as in: = stats = %s --as=ratio --floor=mean)\n", indent, name);
	fprintf (f, "%s  --minsd=<value|variable> use max(stddev, this) as the stddev of --as=stddev and zscore\n", indent);
	}

dspop* op_localstats_parse (char* name, int argc, char** argv)
	{
	dspop_localstats* op = (dspop_localstats*) new_op (name, sizeof(dspop_localstats), false);
	op->windowSize = (u32) get_named_global ("windowSize", 100);
	op->what       = GDSP_LOCALSTATS_ZSCORE;
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
				chastise ("[%s] --as must be zscore, mean, variance, stddev, difference or ratio (\"%s\")\n", name, arg);
			op->what = figures[k].what;
			continue;
			}
		if (strcmp_prefix (arg, "--floor=") == 0)
			{ level_arg (name, arg, argVal, &op->floor, &op->floorVarName);  op->haveFloor = true;  continue; }
		if (strcmp_prefix (arg, "--minsd=") == 0)
			{ level_arg (name, arg, argVal, &op->minSd, &op->minSdVarName);  op->haveMinSd = true;  continue; }
		if (strcmp (arg, "--debug") == 0) continue;
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->windowSize > GDSP_LOCALSTATS_MAX_WINDOW)
		chastise ("[%s] window size %u is above the largest this operator supports (%d)\n",
		          name, op->windowSize, GDSP_LOCALSTATS_MAX_WINDOW);
	return (dspop*) op;
	}

void op_localstats_free (dspop* _op)
	{
	dspop_localstats* op = (dspop_localstats*) _op;
	if (op->floorVarName != NULL) free (op->floorVarName);
	if (op->minSdVarName != NULL) free (op->minSdVarName);
	free (op);
	}

/* the variables are fetched when the operator first runs: by then `stats` or `percentile` has set them */
static void resolve_levels (dspop_localstats* op)
	{
	resolve_variable (&op->common, &op->floorVarName, &op->floor, "floor");
	resolve_variable (&op->common, &op->minSdVarName, &op->minSd, "smallest stddev");
	}

void op_localstats_apply (dspop* _op, char* vName, u32 vLen, valtype* v)
	{
	dspop_localstats* op = (dspop_localstats*) _op;
	resolve_levels (op);
	check_gdsp (gdsp_localstats (v, partner_vector (vName), vLen, op->windowSize, op->what,
	                             op->haveFloor, op->floor, op->haveMinSd, op->minSd, op_stream ()), _op->name);
	flip_vector (vName);
	}

/* the driver: slidingsum's window, [c-lft, c+rgt] with the longer side on the left, and one launch per device (windows
 * above the maximum were refused at parse time) */
static int localstats_reach (dspop* op, u32* left, u32* right) { return reach_centred (((dspop_localstats*) op)->windowSize, right, left); }

static int localstats_batch (dspop* _op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	dspop_localstats* op = (dspop_localstats*) _op;
	resolve_levels (op);
	return gdsp_localstats_batch (items, nitems, op->windowSize, op->what,
	                              op->haveFloor, op->floor, op->haveMinSd, op->minSd, stream);
	}

static const dspinfo localstatsRows[] =
	{ dspinforecord("localstats", op_localstats), dspinfoalias ("local_stats"), dspinfoalias ("localzscore"),
	  dspinfoalias ("localbackground") };
static const optraits localstatsTraits[] = { { op_localstats_apply, false, false, localstats_reach, localstats_batch, NULL } };
const opgroup opgroup_localstats = OPGROUP (localstatsRows, localstatsTraits, NULL);
