/* ops_percentilesover.c -- percentilesover and medianover (device shims).  Not operators of the reference: a table with one
 * line per interval of a file -- the size of the interval's sample and the exact median, or any list of percentiles, of
 * the signal inside it (median depth per exon, gene or bin; quartiles per peak; a per-region background that one tower of
 * reads does not drag).  What statsover leaves out, since it takes more than one reduction per interval.  The signal is
 * not modified and no variable is set.  The two operators differ in name only: both default to --percentiles=50.
 *
 * The file is read, the intervals are batched and the lines are written by the half shared with statsover and
 * breadthover, which also takes the options the three have in common (interval_table_run, interval_op: ops_common.c;
 * host_services.h says how): the intervals may overlap and come in any order, and every ib_batch_limit() of them, and at
 * the end of the file, each device answers the intervals on its chromosomes in one call (gdsp_interval_percentiles_batch,
 * include/genodsp_hip.h: every value an input value, a function of the interval's sample alone).  What is these
 * operators' own is that call, the header with a column per percentile and the values of a line, NA where the sample is
 * empty.
 *
 * The driver finds these operators through opgroup_percentilesover, at the end of this file (host_services.h); every call
 * into the device library for them stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_percentilesover)  dspprototypes(op_medianover)

typedef struct dspop_percentilesover
	{
	interval_op head;
	u32         pcts[GDSP_INTERVAL_PERCENTILES_MAX];   /* thousandths of a percent, in the order given */
	int         numPcts;
	} dspop_percentilesover;

static void percentilesover_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sPrint one line per interval of a file, in file order: chromosome, start, end, then the\n", indent);
	fprintf (f, "%snumber of values looked at and, for every percentile asked for, the value of that rank among\n", indent);
	fprintf (f, "%sthem (percentile's order and rank rule; 50 is the upper median of an even count). Every value\n", indent);
	fprintf (f, "%sis one of the interval's own. Intervals may overlap and come in any order. An interval with\n", indent);
	fprintf (f, "%snothing to look at prints 0 and NA. The signal is not modified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> [options]\n", indent, name);
	fprintf (f, "%s  --percentiles=<p>[,<p>...]  0 to 100 each, in steps of 0.001, at most %d (default: 50)\n", indent, GDSP_INTERVAL_PERCENTILES_MAX);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout, when the operator runs)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        coordinate convention of the file\n", indent);
	}

static void take_percentiles (dspop_percentilesover* op, char* name, char* arg, char* list)
	{
	char* text = copy_string (list);
	op->numPcts = 0;
	for (char* t=text ; t!=NULL ; )
		{
		char* comma = strchr (t, ',');
		if (comma != NULL) *(comma++) = 0;
		valtype pct;
		if (!try_string_to_valtype (t, &pct)) chastise ("[%s] \"%s\" is not a percentile (\"%s\")\n", name, t, arg);
		if (!((pct >= 0.0) && (pct <= 100.0))) chastise ("[%s] percentile must be between 0 and 100 (\"%s\")\n", name, arg);
		if (op->numPcts == GDSP_INTERVAL_PERCENTILES_MAX)
			chastise ("[%s] at most %d percentiles can be asked for (\"%s\")\n", name, GDSP_INTERVAL_PERCENTILES_MAX, arg);
		op->pcts[op->numPcts++] = to_thousandths (pct);
		t = comma;
		}
	free (text);
	}

static dspop* percentilesover_parse (char* name, int argc, char** argv)
	{
	dspop_percentilesover* op = (dspop_percentilesover*) new_op (name, sizeof(dspop_percentilesover), true);
	interval_op_init (&op->head);
	op->pcts[0] = 50000;  op->numPcts = 1;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		if ((strcmp_prefix (arg, "--percentiles=") == 0) || (strcmp_prefix (arg, "--percentile=") == 0))
			take_percentiles (op, name, arg, strchr (arg, '=') + 1);
		else
			interval_op_take (&op->head, name, arg);
		}
	interval_op_check (&op->head, name);
	return (dspop*) op;
	}

static void percentilesover_free (dspop* op)
	{
	interval_op_free ((interval_op*) op);
	free (op);
	}

/* ------------------------------------------------------------------------------------- the table's figures ---- */
/* what is kept of an interval: the size of its sample and, in the order asked for, its numPcts percentiles */
typedef struct pctrec { u32 count;  double values[]; } pctrec;
#define pctrec_size(np) counted_figures_size (np, sizeof(double))
_Static_assert (__builtin_offsetof (pctrec, count) == 0 && __builtin_offsetof (pctrec, values) == sizeof(double), "counted_figures' record");

/* one device's share in one call */
static void answer_percentiles (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out)
	{
	dspop_percentilesover* op = (dspop_percentilesover*) ctx;
	char* name = op->head.common.name;
	counted_figures f = counted_figures_new (name, k, (size_t) op->numPcts, sizeof(double));
	check_gdsp (gdsp_interval_percentiles_batch (items, m, vec, start, end, k, op->pcts, op->numPcts, op->head.sample.minAllowed,
	                                             op->head.sample.maxAllowed, f.count, (double*) f.figures, op_stream ()), name);
	counted_figures_into (&f, out);
	}

/* a line: the name, two coordinates and the count (at most 20 digits each), np values of at most 400 characters, tabs */
#define pct_line_max(np) (100 + 401 * (size_t) (np))

static char* put_percentiles (void* ctx, char* p, const void* rec, arg_dont_complain(spec* s))
	{
	dspop_percentilesover* op = (dspop_percentilesover*) ctx;
	const pctrec* r = (const pctrec*) rec;
	*(p++) = '\t';
	p = put_unsigned (p, r->count);
	for (int j=0 ; j<op->numPcts ; j++)
		{
		const double x = r->values[j];
		*(p++) = '\t';
		if (isnan (x)) { *(p++) = 'N';  *(p++) = 'A'; }
		else           p = put_value (p, x, op->head.sample.precision);
		}
	*(p++) = '\n';
	return p;
	}

/* the header: a column per percentile, named as percentile names its variable */
static void put_header (void* ctx, FILE* out)
	{
	dspop_percentilesover* op = (dspop_percentilesover*) ctx;
	fputs ("#chrom\tstart\tend\tcount", out);
	for (int j=0 ; j<op->numPcts ; j++)
		{
		char varName[200];
		percentile_name (varName, op->pcts[j]);
		fprintf (out, "\tp%s", varName + strlen ("percentile"));
		}
	fputc ('\n', out);
	}

static void percentilesover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_percentilesover* op = (dspop_percentilesover*) _op;
	interval_table t = { pctrec_size (op->numPcts), answer_percentiles, put_percentiles, pct_line_max (op->numPcts), put_header, op, 0, 0, 0, 0 };
	interval_op_run (&op->head, &t);
	}

/* (the work trait's 8 B per base: the long route reads an interval once per digit it needs, so a lower bound there) */
OP_SHORT (op_percentilesover, "print the exact percentiles of the signal over each interval of a file (not in genodsp)")
void   op_percentilesover_usage (char* name, FILE* f, char* indent) { percentilesover_usage (name, f, indent); }
dspop* op_percentilesover_parse (char* name, int argc, char** argv) { return percentilesover_parse (name, argc, argv); }
void   op_percentilesover_free  (dspop* op) { percentilesover_free (op); }
void   op_percentilesover_apply (dspop* op, char* vName, u32 vLen, valtype* v) { percentilesover_apply (op, vName, vLen, v); }

OP_SHORT (op_medianover, "print the exact median of the signal over each interval of a file (not in genodsp)")
void   op_medianover_usage (char* name, FILE* f, char* indent) { percentilesover_usage (name, f, indent); }
dspop* op_medianover_parse (char* name, int argc, char** argv) { return percentilesover_parse (name, argc, argv); }
void   op_medianover_free  (dspop* op) { percentilesover_free (op); }
void   op_medianover_apply (dspop* op, char* vName, u32 vLen, valtype* v) { percentilesover_apply (op, vName, vLen, v); }

static const dspinfo percentilesoverRows[] =
	{ dspinforecord("percentilesover", op_percentilesover), dspinfoalias ("percentiles_over"), dspinfoalias ("quantilesover"),
	  dspinfoalias ("interval_percentiles"),
	  dspinforecord("medianover", op_medianover), dspinfoalias ("median_over") };
static const optraits percentilesoverTraits[] =
	{ { op_percentilesover_apply, true, false, NULL, NULL, interval_op_work },
	  { op_medianover_apply,      true, false, NULL, NULL, interval_op_work } };
const opgroup opgroup_percentilesover = OPGROUP (percentilesoverRows, percentilesoverTraits, NULL);
