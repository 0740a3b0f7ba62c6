/* ops_stats.c -- stats, normalize, multiplyconst, divideconst (device shims).  Not operators of the reference, which has
 * no genome-wide mean or standard deviation and no way to scale the signal by a variable: depth over mean depth, a
 * z-score before `binarize`, reads per million.
 *
 * stats and normalize are whole-genome operators like percentile: they sample the signal by percentile's rules
 * (--window counted from each chromosome's first base, --min / --max) wherever it lives -- whole chromosomes or, under
 * --sharding=bases, the stretches each device answers for -- and set the named variables count, sum, mean, variance
 * and stddev.  Every figure is exact and rounded once (gdsp_genome_stats, include/genodsp_hip.h), so what they print
 * and what normalize writes do not depend on the number of devices, the cut of the genome, chromosome order or the
 * way the devices' images meet (RCCL all-reduce of u64 words, or a host sum with --reduce=host).
 * multiplyconst and divideconst are per-base operators that take a number or a variable.
 *
 * The driver finds these operators through opgroup_stats, at the end of this file (host_services.h); every call into the
 * device library for them stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_stats)  dspprototypes(op_normalize)  dspprototypes(op_multiply_constant)  dspprototypes(op_divide_constant)

/* ---------------------------------------------------------------------------------------- stats, normalize ---- */
typedef struct dspop_stats
	{
	dspop       common;
	sample_opts sample;                         /* (as percentile) */
	int         reportForBash, zscore;
	} dspop_stats;

static dspop* stats_parse (char* name, int argc, char** argv, int isNormalize)
	{
	dspop_stats* op = (dspop_stats*) new_op (name, sizeof(dspop_stats), true);
	const int accepts = SAMPLE_OPT_WINDOW | SAMPLE_OPT_QUIET | (isNormalize? 0 : SAMPLE_OPT_PRECISION);
	sample_opts_init (&op->sample);
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (sample_opts_take (&op->sample, name, arg, accepts)) continue;
		if (isNormalize && (strcmp_prefix (arg, "--to=") == 0))
			{
			if      (strcmp (argVal, "mean")   == 0) op->zscore = false;
			else if (strcmp (argVal, "zscore") == 0) op->zscore = true;
			else chastise ("[%s] unknown --to=%s (mean or zscore)\n", name, argVal);
			continue;
			}
		if (!isNormalize && ((strcmp (arg, "--report:bash") == 0) || (strcmp (arg, "--bash") == 0))) { op->reportForBash = true;  continue; }
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->reportForBash && op->sample.quiet) chastise ("[%s] Can't use both --report:bash and --quiet\n", name);
	return (dspop*) op;
	}

static void stats_usage (char* name, FILE* f, char* indent, int isNormalize)
	{
	if (indent == NULL) indent = "";
	if (isNormalize)
		{
		fprintf (f, "%sDivide every base by the genome-wide mean, or turn it into a z-score. Sets the\n", indent);
		fprintf (f, "%svariables stats sets. Not in genodsp.\n\n", indent);
		fprintf (f, "%susage: %s [options]\n", indent, name);
		fprintf (f, "%s  --to=mean|zscore         v/mean (default) or (v-mean)/stddev\n", indent);
		}
	else
		{
		fprintf (f, "%sCompute the count, sum, mean, variance and standard deviation of the values over\n", indent);
		fprintf (f, "%sall chromosomes, each exact and rounded once; each is stored in a named variable\n", indent);
		fprintf (f, "%s(count, sum, mean, variance, stddev). The signal is not modified. Not in genodsp.\n\n", indent);
		fprintf (f, "%susage: %s [options]\n", indent, name);
		}
	fprintf (f, "%s  --window=<length>        (W=) look at one base per window\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	if (!isNormalize)
		{
		fprintf (f, "%s  --precision=<number>     digits after the point when reporting (default: all of them)\n", indent);
		fprintf (f, "%s  --report:bash            print results as shell assignments on stdout\n", indent);
		}
	fprintf (f, "%s  --quiet                  do not report results on stderr\n", indent);
	}

/* the figures of the sampled genome, over every device (and every rank of the reduction hook); sets the variables */
static void stats_compute (dspop_stats* op, double* fig)
	{
	gdsp_xsum_source* src;
	int nsrc = signal_sources (op->common.name, &src);
	void* reduceCtx = NULL;
	gdsp_reduce_fn reduce = reduce_over_devices (&reduceCtx);    /* (also hands the communicator to the library) */
	check_gdsp (gdsp_genome_stats (src, nsrc, op->sample.window, op->sample.minAllowed, op->sample.maxAllowed, reduce, reduceCtx, fig),
	            op->common.name);
	free (src);
	static char* names[5] = { "count", "sum", "mean", "variance", "stddev" };
	for (int k=0 ; k<5 ; k++)
		{
		if ((fig[0] == 0) && (k >= 2)) continue;                 /* (no mean of nothing) */
		set_named_global (names[k], fig[k]);
		if (op->sample.quiet) continue;
		char text[400];
		format_value (text, sizeof(text), fig[k], op->sample.precision);
		if (op->reportForBash) fprintf (stdout, "%s=%s # bash command\n", names[k], text);
		else                   fprintf (stderr, "%s is %s\n", names[k], text);
		}
	}

OP_SHORT (op_stats, "compute the genome-wide count, sum, mean, variance and stddev (not in genodsp)")
void   op_stats_usage (char* name, FILE* f, char* indent) { stats_usage (name, f, indent, false); }
dspop* op_stats_parse (char* name, int argc, char** argv) { return stats_parse (name, argc, argv, false); }
void   op_stats_free  (dspop* op) { free (op); }

void op_stats_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	double fig[5];
	stats_compute ((dspop_stats*) _op, fig);
	if (fig[0] == 0)
		fprintf (stderr, "[%s] stats can't be computed;  no input values meet the criteria\n", _op->name);
	}

OP_SHORT (op_normalize, "divide by the genome-wide mean, or make z-scores (not in genodsp)")
void   op_normalize_usage (char* name, FILE* f, char* indent) { stats_usage (name, f, indent, true); }
dspop* op_normalize_parse (char* name, int argc, char** argv) { return stats_parse (name, argc, argv, true); }
void   op_normalize_free  (dspop* op) { free (op); }

/* every base of every part, halo included (base / baseLen): the halos stay their neighbours' bases */
void op_normalize_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_stats* op = (dspop_stats*) _op;
	double fig[5];
	stats_compute (op, fig);
	if (fig[0] == 0)
		{ fprintf (stderr, "[%s] can't normalize;  no input values meet the criteria\n", _op->name);  exit (EXIT_FAILURE); }
	const double div = op->zscore? fig[4] : fig[2];
	const char*  what = op->zscore? "standard deviation" : "mean";
	if (!((div != 0) && (fabs (div) <= DBL_MAX)))
		{ fprintf (stderr, "[%s] can't normalize;  the %s is %.17g\n", _op->name, what, div);  exit (EXIT_FAILURE); }
	sigpart* parts;
	int nparts = signal_parts (&parts);
	gdsp_batch_item* items = (gdsp_batch_item*) calloc (nparts? nparts : 1, sizeof(gdsp_batch_item));
	if (items == NULL) { fprintf (stderr, "[%s] out of memory\n", _op->name);  exit (EXIT_FAILURE); }
	for (int d=0 ; d<device_count_in_use () ; d++)             /* one launch per device */
		{
		int m = 0;
		spec* first = NULL;
		for (int i=0 ; i<nparts ; i++)
			{
			if (device_index_of (parts[i].s) != d) continue;
			if (first == NULL) first = parts[i].s;
			items[m].d_in = NULL;  items[m].d_out = parts[i].base;  items[m].n = parts[i].baseLen;  m++;
			}
		if (m == 0) continue;
		select_device_of (first);
		if (op->zscore) check_gdsp (gdsp_standardize_batch (items, m, fig[2], div, op_stream ()), _op->name);
		else            check_gdsp (gdsp_divide_constant_batch (items, m, div, op_stream ()), _op->name);
		}
	if (nparts > 0) select_device_of (parts[0].s);
	free (items);
	}

/* ---------------------------------------------------------------------------- multiplyconst, divideconst ---- */
typedef struct dspop_const { dspop common;  char* varName;  valtype val; } dspop_const;

static dspop* const_parse (char* name, int argc, char** argv, int isDivide)
	{
	dspop_const* op = (dspop_const*) new_op (name, sizeof(dspop_const), false);
	int haveVal = false;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		if ((strcmp_prefix (arg, "--") == 0) || haveVal) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		value_or_variable (arg, &op->val, &op->varName);
		haveVal = true;
		}
	if (!haveVal) chastise ("[%s] no constant value was provided\n", name);
	if (isDivide && (op->varName == NULL) && (op->val == 0)) chastise ("[%s] can't divide by zero\n", name);
	return (dspop*) op;
	}

static void const_free (dspop* _op)
	{
	dspop_const* op = (dspop_const*) _op;
	if (op->varName != NULL) free (op->varName);
	free (op);
	}

/* the constant, its variable resolved on first use (a variable that holds 0 is refused for divideconst) */
static valtype const_value (dspop* _op)
	{
	dspop_const* op = (dspop_const*) _op;
	resolve_variable (_op, &op->varName, &op->val, "constant");
	if ((_op->funcApply == op_divide_constant_apply) && (op->val == 0))
		{ fprintf (stderr, "[%s] can't divide by zero\n", _op->name);  exit (EXIT_FAILURE); }
	return op->val;
	}

OP_SHORT (op_multiply_constant, "multiply the current set of interval values by a constant (not in genodsp)")

void op_multiply_constant_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sMultiply every base by a constant. Not in genodsp.\n\n%susage: %s <value|variable>\n", indent, indent, name);
	}

dspop* op_multiply_constant_parse (char* name, int argc, char** argv) { return const_parse (name, argc, argv, false); }
void   op_multiply_constant_free  (dspop* op) { const_free (op); }

void op_multiply_constant_apply (dspop* _op, arg_dont_complain(char* vName), u32 vLen, valtype* v)
	{ valtype c = const_value (_op);  check_gdsp (gdsp_multiply_constant (v, vLen, c, op_stream ()), _op->name); }

OP_SHORT (op_divide_constant, "divide the current set of interval values by a constant (not in genodsp)")

void op_divide_constant_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sDivide every base by a constant (not zero). Not in genodsp.\n\n%susage: %s <value|variable>\n", indent, indent, name);
	}

dspop* op_divide_constant_parse (char* name, int argc, char** argv) { return const_parse (name, argc, argv, true); }
void   op_divide_constant_free  (dspop* op) { const_free (op); }

void op_divide_constant_apply (dspop* _op, arg_dont_complain(char* vName), u32 vLen, valtype* v)
	{ valtype c = const_value (_op);  check_gdsp (gdsp_divide_constant (v, vLen, c, op_stream ()), _op->name); }

/* the driver: multiplyconst and divideconst are per-base and in place, with one launch per device; stats and normalize
 * take the signal's parts as they are (normalize rewrites halo and owner alike), at 8 B per base and stats pass */
static int const_batch (dspop* op, const gdsp_batch_item* items, int nitems, void* stream)
	{
	valtype c = const_value (op);
	if (op->funcApply == op_multiply_constant_apply) return gdsp_multiply_constant_batch (items, nitems, c, stream);
	return gdsp_divide_constant_batch (items, nitems, c, stream);
	}

static void stats_work     (dspop* op, u64* bases, double* bytesPerBase) { *bytesPerBase = 16; }
static void normalize_work (dspop* op, u64* bases, double* bytesPerBase) { *bytesPerBase = 32; }

static const dspinfo statsRows[] =
	{ dspinforecord("stats"         , op_stats)            ,
	  dspinforecord("normalize"     , op_normalize)        ,
	  dspinforecord("multiplyconst" , op_multiply_constant), dspinfoalias ("multiply_const"), dspinfoalias ("scale"),
	  dspinforecord("divideconst"   , op_divide_constant)  , dspinfoalias ("divide_const") };
static const optraits statsTraits[] =
	{ { op_stats_apply,             true, true,  NULL,       NULL,        stats_work },
	  { op_normalize_apply,         true, true,  NULL,       NULL,        normalize_work },
	  { op_multiply_constant_apply, true, false, reach_none, const_batch, NULL },
	  { op_divide_constant_apply,   true, false, reach_none, const_batch, NULL } };
const opgroup opgroup_stats = OPGROUP (statsRows, statsTraits, gdsp_genome_stats_use_comm);
