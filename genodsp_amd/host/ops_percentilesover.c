/* ops_percentilesover.c -- percentilesover and medianover (device shims).  Not operators of the reference: a table with one
 * line per interval of a file -- the size of the interval's sample and the exact median, or any list of percentiles, of
 * the signal inside it (median depth per exon, gene or bin; quartiles per peak; a per-region background that one tower of
 * reads does not drag).  What statsover leaves out, since it takes more than one reduction per interval.  The signal is
 * not modified and no variable is set.  The two operators differ in name only: both default to --percentiles=50.
 *
 * The file is read, the intervals are batched and the lines are written by the half shared with statsover
 * (interval_table_run, ops_common.c; host_services.h says how): the intervals may overlap and come in any order, and every
 * ib_batch_limit() of them, and at the end of the file, each device answers the intervals on its chromosomes in one call
 * (gdsp_interval_percentiles_batch, include/genodsp_hip.h: every value an input value, a function of the interval's sample
 * alone).  What is these operators' own is that call, the header with a column per percentile and the values of a line,
 * NA where the sample is empty.
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
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                         /* (its limits and precision; no window) */
	int         originOne;
	u32         pcts[GDSP_INTERVAL_PERCENTILES_MAX];   /* thousandths of a percent, in the order given */
	int         numPcts;
	u64         bases;                          /* summed length of the intervals (--report=gpu) */
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
	sample_opts_init (&op->sample);
	op->originOne = (int) get_named_global ("originOne", false);
	op->pcts[0] = 50000;  op->numPcts = 1;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if ((strcmp_prefix (arg, "--percentiles=") == 0) || (strcmp_prefix (arg, "--percentile=") == 0))
			{ take_percentiles (op, name, arg, argVal);  continue; }
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

static void percentilesover_free (dspop* _op)
	{
	dspop_percentilesover* op = (dspop_percentilesover*) _op;
	if (op->filename    != NULL) free (op->filename);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

/* ------------------------------------------------------------------------------------- the table's figures ---- */
/* what is kept of an interval: the size of its sample and, in the order asked for, its numPcts percentiles */
typedef struct pctrec { u32 count;  double values[]; } pctrec;
#define pctrec_size(np) (sizeof(pctrec) + (size_t) (np) * sizeof(double))

/* one device's share in one call */
static void answer_percentiles (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out)
	{
	dspop_percentilesover* op = (dspop_percentilesover*) ctx;
	char*        name = op->common.name;
	const size_t np = (size_t) op->numPcts;
	u32*    count  = (u32*) must_alloc (malloc (k * sizeof(u32)), name);
	double* values = (double*) must_alloc (malloc (k * np * sizeof(double)), name);
	check_gdsp (gdsp_interval_percentiles_batch (items, m, vec, start, end, k, op->pcts, op->numPcts, op->sample.minAllowed,
	                                             op->sample.maxAllowed, count, values, op_stream ()), name);
	for (size_t i=0 ; i<k ; i++)
		{
		pctrec* r = (pctrec*) ((char*) out + i * pctrec_size (np));
		r->count = count[i];
		memcpy (r->values, &values[i * np], np * sizeof(double));
		}
	free (count);  free (values);
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
		else           p = put_value (p, x, op->sample.precision);
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
	interval_table_run (_op->name, op->filename, op->outFilename, op->originOne, &t);
	op->bases += t.bases;
	}

/* the driver: the signal is only read, 8 B per base of the intervals' summed length since the last call (the long
 * route reads an interval once per digit it needs: a lower bound there) */
static void percentilesover_work (dspop* op, u64* bases, double* bytesPerBase)
	{ *bases = ((dspop_percentilesover*) op)->bases;  ((dspop_percentilesover*) op)->bases = 0;  *bytesPerBase = 8; }

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
	{ { op_percentilesover_apply, true, false, NULL, NULL, percentilesover_work },
	  { op_medianover_apply,      true, false, NULL, NULL, percentilesover_work } };
const opgroup opgroup_percentilesover = OPGROUP (percentilesoverRows, percentilesoverTraits, NULL);
