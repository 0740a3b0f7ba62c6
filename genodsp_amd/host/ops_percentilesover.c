/* ops_percentilesover.c -- percentilesover and medianover (device shims).  Not operators of the reference: a table with one
 * line per interval of a file -- the size of the interval's sample and the exact median, or any list of percentiles, of
 * the signal inside it (median depth per exon, gene or bin; quartiles per peak; a per-region background that one tower of
 * reads does not drag).  What statsover leaves out, since it takes more than one reduction per interval.  The signal is
 * not modified and no variable is set.  The two operators differ in name only: both default to --percentiles=50.
 *
 * The file is read like statsover's (ops_statsover.c: read_interval without a value column, the routing, origin and
 * clipping rules of fileop_apply; the intervals may overlap and come in any order), buffered with ib_add -- the value slot
 * carries the interval's serial number in its batch -- and every ib_batch_limit() of them, and at the end of the file,
 * each device answers the intervals on its chromosomes in one call (gdsp_interval_percentiles_batch,
 * include/genodsp_hip.h: every value an input value, a function of the interval's sample alone).  Batches are
 * consecutive stretches of the file, so printing them one after the other keeps file order.
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

/* ------------------------------------------------------------------------------------------ one batch ---- */
/* a kept interval as its line names it; its figures arrive in count[] and values[] under the same serial number */
typedef struct row { spec* s;  u32 fileStart, fileEnd; } row;

typedef struct batch
	{
	row*   rows;   u32* count;   double* values;   size_t cap;                /* by serial number */
	u32   *vec, *start, *end, *serial, *outCount;  double* outValues;  size_t ivCap;   /* one device's share, as the library takes it */
	char*  text;   size_t textCap;
	} batch;

/* the pending intervals' figures, device by device (one call each), then their lines in file order */
static void flush_batch (dspop_percentilesover* op, batch* b, u64 pending, FILE* f)
	{
	const char*  name = op->common.name;
	const int    numChroms = ib_chromosomes ();
	const size_t np = (size_t) op->numPcts;
	if (pending == 0) return;
	gdsp_batch_item* items = (gdsp_batch_item*) must_alloc (calloc (numChroms + 1, sizeof(gdsp_batch_item)), name);
	sync_all_devices ();
	for (int d=0 ; d<device_count_in_use () ; d++)
		{
		int    m = 0;
		size_t k = 0, want = 0;
		spec*  first = NULL;
		for (int ci=0 ; ci<numChroms ; ci++)
			{
			spec* s;  u32 *start, *end;  valtype* val;
			u32 count = ib_pending_of (ci, &s, &start, &end, &val);
			if ((count != 0) && (device_index_of (s) == d)) want += count;
			}
		if (want == 0) continue;
		if (want > b->ivCap)
			{
			free (b->vec);  free (b->start);  free (b->end);  free (b->serial);  free (b->outCount);  free (b->outValues);
			b->vec       = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->start     = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->end       = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->serial    = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->outCount  = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->outValues = (double*) must_alloc (malloc (want * GDSP_INTERVAL_PERCENTILES_MAX * sizeof(double)), name);
			b->ivCap     = want;
			}
		for (int ci=0 ; ci<numChroms ; ci++)
			{
			spec* s;  u32 *start, *end;  valtype* val;
			u32 count = ib_pending_of (ci, &s, &start, &end, &val);
			if ((count == 0) || (device_index_of (s) != d)) continue;
			if (first == NULL) first = s;
			items[m].d_in = s->valVector;  items[m].d_out = NULL;  items[m].n = s->length;
			for (u32 i=0 ; i<count ; i++, k++)
				{ b->vec[k] = (u32) m;  b->start[k] = start[i];  b->end[k] = end[i];  b->serial[k] = (u32) val[i]; }
			m++;
			}
		select_device_of (first);
		check_gdsp (gdsp_interval_percentiles_batch (items, m, b->vec, b->start, b->end, (u32) k, op->pcts, op->numPcts,
		                                             op->sample.minAllowed, op->sample.maxAllowed, b->outCount, b->outValues,
		                                             op_stream ()), name);
		for (size_t i=0 ; i<k ; i++)
			{
			b->count[b->serial[i]] = b->outCount[i];
			memcpy (&b->values[b->serial[i] * np], &b->outValues[i * np], np * sizeof(double));
			}
		}
	free (items);
	select_device_of (chromsSorted[0]);

	/* a line: the name, two coordinates and the count (at most 20 digits each), np values of at most 400 characters, tabs */
	const size_t lineMax = 100 + 401 * np;
	size_t len = 0;
	for (u64 r=0 ; r<pending ; r++)
		{
		const row* w = &b->rows[r];
		const size_t chromLen = strlen (w->s->chrom);
		if (len + chromLen + lineMax > b->textCap)
			{
			if (len != 0) { fwrite (b->text, 1, len, f);  len = 0; }
			if (chromLen + lineMax > b->textCap)
				{
				b->textCap = (1u << 20) + chromLen + lineMax;
				b->text = (char*) must_alloc (realloc (b->text, b->textCap), name);
				}
			}
		char* p = b->text + len;
		memcpy (p, w->s->chrom, chromLen);  p += chromLen;  *(p++) = '\t';
		p = put_unsigned (p, w->fileStart);  *(p++) = '\t';
		p = put_unsigned (p, w->fileEnd);    *(p++) = '\t';
		p = put_unsigned (p, b->count[r]);
		for (size_t j=0 ; j<np ; j++)
			{
			const double x = b->values[r * np + j];
			*(p++) = '\t';
			if (isnan (x)) { *(p++) = 'N';  *(p++) = 'A'; }
			else           p = put_value (p, x, op->sample.precision);
			}
		*(p++) = '\n';
		len = (size_t) (p - b->text);
		}
	if (len != 0) fwrite (b->text, 1, len, f);
	ib_begin ();                                               /* forget them */
	}

static void percentilesover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_percentilesover* op = (dspop_percentilesover*) _op;
	char    line[1001], prevChrom[1001];
	char*   chrom;
	spec*   s = NULL;
	u32     start, end, o = op->originOne? 1 : 0;
	valtype val;
	batch   b;
	memset (&b, 0, sizeof(b));

	FILE* f = fopen (op->filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", _op->name, op->filename);  exit (EXIT_FAILURE); }
	FILE* out = open_table (_op->name, op->outFilename);
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;

	/* the header: a column per percentile, named as percentile names its variable */
	fputs ("#chrom\tstart\tend\tcount", out);
	for (int j=0 ; j<op->numPcts ; j++)
		{
		char varName[200];
		percentile_name (varName, op->pcts[j]);
		fprintf (out, "\tp%s", varName + strlen ("percentile"));
		}
	fputc ('\n', out);

	ib_begin ();
	prevChrom[0] = 0;
	while (read_interval (f, line, sizeof(line), /*valCol*/ -1, &chrom, &start, &end, &val))
		{
		if (strcmp (chrom, prevChrom) != 0)
			{ s = find_chromosome_spec (chrom);  safe_strncpy (prevChrom, chrom, sizeof(prevChrom)-1); }
		if (s == NULL) continue;
		if (!s->flag) { if (trackOperations) fprintf (stderr, "%s(%s)\n", _op->name, chrom);  s->flag = true; }

		const u32 fileStart = start;
		start -= o;
		u32 adjStart, adjEnd;
		if (!place_interval (_op->name, op->filename, chrom, s, start, end, &adjStart, &adjEnd)) continue;
		if (adjStart >= adjEnd) continue;                      /* (an empty interval has no sample and no line) */
		const u64 serial = ib_pending ();
		if (serial >= b.cap)
			{
			b.cap    = (b.cap == 0)? 4096 : 2*b.cap;
			b.rows   = (row*) must_alloc (realloc (b.rows, b.cap * sizeof(row)), _op->name);
			b.count  = (u32*) must_alloc (realloc (b.count, b.cap * sizeof(u32)), _op->name);
			b.values = (double*) must_alloc (realloc (b.values, b.cap * GDSP_INTERVAL_PERCENTILES_MAX * sizeof(double)), _op->name);
			}
		b.rows[serial].s = s;  b.rows[serial].fileStart = fileStart;  b.rows[serial].fileEnd = end;
		ib_add (s, adjStart, adjEnd, (valtype) serial);
		op->bases += adjEnd - adjStart;
		if (ib_pending () >= ib_batch_limit ()) flush_batch (op, &b, ib_pending (), out);
		}
	fclose (f);
	flush_batch (op, &b, ib_pending (), out);
	close_table (out);
	free (b.rows);  free (b.count);  free (b.values);  free (b.vec);  free (b.start);  free (b.end);  free (b.serial);
	free (b.outCount);  free (b.outValues);  free (b.text);
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
