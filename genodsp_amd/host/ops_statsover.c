/* ops_statsover.c -- statsover (device shim).  Not an operator of the reference: a table with one line per interval of a
 * file -- count, sum, mean, min, max and the position of the maximum of the signal inside it (mean depth per gene;
 * height, area and summit of every peak; signal per bin).  The signal is not modified and no variable is set.
 *
 * The file is read, the intervals are batched and the lines are written by the half shared with percentilesover and
 * breadthover, which also takes the options the three have in common (interval_table_run, interval_op: ops_common.c;
 * host_services.h says how): the intervals may overlap and come in any order, and every ib_batch_limit() of them, and at
 * the end of the file, each device computes the figures of the intervals on its chromosomes in one launch
 * (gdsp_interval_stats_batch, include/genodsp_hip.h: every figure exact and rounded once, a function of the interval's
 * sample alone).  What is statsover's own is that call, the figures of a line (put_interval_figures) and, with
 * GDSP_STATSOVER_TIMES=1, where a run's time went, on stderr.
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

typedef struct dspop_statsover { interval_op head; } dspop_statsover;

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
	interval_op_init (&op->head);
	for ( ; argc > 0 ; argv++, argc--) interval_op_take (&op->head, name, argv[0]);
	interval_op_check (&op->head, name);
	return (dspop*) op;
	}

void op_statsover_free (dspop* op)
	{
	interval_op_free ((interval_op*) op);
	free (op);
	}

/* ------------------------------------------------------------------------------------- the table's figures ---- */
/* one device's share in one launch */
static void answer_stats (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out)
	{
	dspop_statsover* op = (dspop_statsover*) ctx;
	check_gdsp (gdsp_interval_stats_batch (items, m, vec, start, end, k, op->head.sample.minAllowed, op->head.sample.maxAllowed,
	                                       (gdsp_interval_stat*) out, op_stream ()), op->head.common.name);
	}

static char* put_stats (void* ctx, char* p, const void* rec, spec* s)
	{
	dspop_statsover* op = (dspop_statsover*) ctx;
	return put_interval_figures (p, (const gdsp_interval_stat*) rec, s->start, op->head.originOne, op->head.sample.precision);
	}

void op_statsover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_statsover* op = (dspop_statsover*) _op;
	interval_table t = { sizeof(gdsp_interval_stat), answer_stats, put_stats, 2200, NULL, op, 0, 0, 0, 0 };
	interval_op_run (&op->head, &t);
	if (getenv ("GDSP_STATSOVER_TIMES") != NULL)
		fprintf (stderr, "[%s] times: %.1f ms = read and route %.1f + device calls %.1f + format and write %.1f\n", _op->name, t.msAll,
		         t.msAll - t.msDevice - t.msFormat, t.msDevice, t.msFormat);
	}

static const dspinfo statsoverRows[] =
	{ dspinforecord("statsover", op_statsover), dspinfoalias ("stats_over"), dspinfoalias ("intervalstats"),
	  dspinfoalias ("interval_stats") };
static const optraits statsoverTraits[] = { { op_statsover_apply, true, false, NULL, NULL, interval_op_work } };
const opgroup opgroup_statsover = OPGROUP (statsoverRows, statsoverTraits, NULL);
