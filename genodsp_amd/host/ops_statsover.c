/* ops_statsover.c -- statsover (device shim).  Not an operator of the reference: a table with one line per interval of a
 * file -- count, sum, mean, min, max and the position of the maximum of the signal inside it (mean depth per gene;
 * height, area and summit of every peak; signal per bin).  The signal is not modified and no variable is set.
 *
 * The file is read, the intervals are batched and the lines are written by the half shared with percentilesover
 * (interval_table_run, ops_common.c; host_services.h says how): the intervals may overlap and come in any order, and every
 * ib_batch_limit() of them, and at the end of the file, each device computes the figures of the intervals on its
 * chromosomes in one launch (gdsp_interval_stats_batch, include/genodsp_hip.h: every figure exact and rounded once, a
 * function of the interval's sample alone).  What is statsover's own is that call, the figures of a line
 * (put_interval_figures) and, with GDSP_STATSOVER_TIMES=1, where a run's time went, on stderr.
 *
 * The driver finds this operator through opgroup_statsover, at the end of this file (host_services.h); every call into the
 * device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_statsover)

typedef struct dspop_statsover
	{
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                         /* (its limits and precision; no window) */
	int         originOne;
	u64         bases;                          /* summed length of the intervals (--report=gpu) */
	} dspop_statsover;

OP_SHORT (op_statsover, "print count, sum, mean, min, max and summit of the signal over each interval of a file (not in genodsp)")

void op_statsover_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sPrint one line per interval of a file, in file order: chromosome, start, end, then the\n", indent);
	fprintf (f, "%scount, sum, mean, min and max of the signal inside the interval and the position of the\n", indent);
	fprintf (f, "%s(first) maximum; sum and mean are exact and rounded once. Intervals may overlap and come in\n", indent);
	fprintf (f, "%sany order. An interval with nothing to look at prints 0, 0 and NA. The signal is not\n", indent);
	fprintf (f, "%smodified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> [options]\n", indent, name);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout, when the operator runs)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        coordinate convention of the file and of the positions printed\n", indent);
	}

dspop* op_statsover_parse (char* name, int argc, char** argv)
	{
	dspop_statsover* op = (dspop_statsover*) new_op (name, sizeof(dspop_statsover), true);
	sample_opts_init (&op->sample);
	op->originOne = (int) get_named_global ("originOne", false);
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if (sample_opts_take (&op->sample, name, arg, SAMPLE_OPT_PRECISION)) continue;
		if (origin_opt_take (arg, &op->originOne)) continue;
		if (strcmp (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (op->filename == NULL) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->filename == NULL) { fprintf (stderr, "[%s] no filename was provided\n", name);  exit (EXIT_FAILURE); }
	if (op->sample.minAllowed > op->sample.maxAllowed) chastise ("[%s] --min can't be above --max\n", name);
	return (dspop*) op;
	}

void op_statsover_free (dspop* _op)
	{
	dspop_statsover* op = (dspop_statsover*) _op;
	if (op->filename    != NULL) free (op->filename);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

/* ------------------------------------------------------------------------------------- the table's figures ---- */
/* one device's share in one launch */
static void answer_stats (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out)
	{
	dspop_statsover* op = (dspop_statsover*) ctx;
	check_gdsp (gdsp_interval_stats_batch (items, m, vec, start, end, k, op->sample.minAllowed, op->sample.maxAllowed,
	                                       (gdsp_interval_stat*) out, op_stream ()), op->common.name);
	}

static char* put_stats (void* ctx, char* p, const void* rec, spec* s)
	{
	dspop_statsover* op = (dspop_statsover*) ctx;
	return put_interval_figures (p, (const gdsp_interval_stat*) rec, s->start, op->originOne, op->sample.precision);
	}

void op_statsover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_statsover* op = (dspop_statsover*) _op;
	interval_table t = { sizeof(gdsp_interval_stat), answer_stats, put_stats, 2200, NULL, op, 0, 0, 0, 0 };
	interval_table_run (_op->name, op->filename, op->outFilename, op->originOne, &t);
	op->bases += t.bases;
	if (getenv ("GDSP_STATSOVER_TIMES") != NULL)
		fprintf (stderr, "[%s] times: %.1f ms = read and route %.1f + device calls %.1f + format and write %.1f\n", _op->name, t.msAll,
		         t.msAll - t.msDevice - t.msFormat, t.msDevice, t.msFormat);
	}

/* the driver: the signal is only read, 8 B per base of the intervals' summed length since the last call */
static void statsover_work (dspop* op, u64* bases, double* bytesPerBase)
	{ *bases = ((dspop_statsover*) op)->bases;  ((dspop_statsover*) op)->bases = 0;  *bytesPerBase = 8; }

static const dspinfo statsoverRows[] =
	{ dspinforecord("statsover", op_statsover), dspinfoalias ("stats_over"), dspinfoalias ("intervalstats"),
	  dspinfoalias ("interval_stats") };
static const optraits statsoverTraits[] = { { op_statsover_apply, true, false, NULL, NULL, statsover_work } };
const opgroup opgroup_statsover = OPGROUP (statsoverRows, statsoverTraits, NULL);
