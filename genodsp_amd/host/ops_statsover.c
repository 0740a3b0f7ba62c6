/* ops_statsover.c -- statsover (device shim).  Not an operator of the reference: a table with one line per interval of a
 * file -- count, sum, mean, min, max and the position of the maximum of the signal inside it (mean depth per gene;
 * height, area and summit of every peak; signal per bin).  The signal is not modified and no variable is set.
 *
 * The file is read like mask's and maxover's (read_interval, no value column; the routing, origin and clipping rules of
 * fileop_apply, ops_intervals.c), but the intervals may overlap and come in any order.  They are buffered with ib_add --
 * the value slot carries the interval's serial number in its batch -- and every ib_batch_limit() of them, and at the end
 * of the file, each device computes the figures of the intervals on its chromosomes in one launch
 * (gdsp_interval_stats_batch, include/genodsp_hip.h: every figure exact and rounded once, a function of the interval's
 * sample alone).  Batches are consecutive stretches of the file, so printing them one after the other keeps file order.
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
	double      msDevice, msFormat;             /* GDSP_STATSOVER_TIMES=1: where a run's time went, on stderr */
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

/* ------------------------------------------------------------------------------------------ one batch ---- */
/* a kept interval as its line names it; its figures arrive in rec[] under the same serial number */
typedef struct row { spec* s;  u32 fileStart, fileEnd; } row;

typedef struct batch
	{
	row*   rows;   gdsp_interval_stat* rec;   size_t cap;  /* by serial number */
	u32   *vec, *start, *end, *serial;  gdsp_interval_stat* out;  size_t ivCap;     /* one device's share, as the library takes it */
	char*  text;   size_t textCap;
	} batch;

/* the pending intervals' figures, device by device (one launch each), then their lines in file order */
static void flush_batch (dspop_statsover* op, batch* b, u64 pending, FILE* f)
	{
	const char* name = op->common.name;
	const int   numChroms = ib_chromosomes ();
	gdsp_batch_item* items = (gdsp_batch_item*) must_alloc (calloc (numChroms + 1, sizeof(gdsp_batch_item)), name);
	if (pending == 0) { free (items);  return; }
	sync_all_devices ();
	const double t0 = now_ms ();
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
			free (b->vec);  free (b->start);  free (b->end);  free (b->serial);  free (b->out);
			b->vec    = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->start  = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->end    = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->serial = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->out    = (gdsp_interval_stat*) must_alloc (malloc (want * sizeof(gdsp_interval_stat)), name);
			b->ivCap  = want;
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
		check_gdsp (gdsp_interval_stats_batch (items, m, b->vec, b->start, b->end, (u32) k, op->sample.minAllowed, op->sample.maxAllowed,
		                                       b->out, op_stream ()), name);
		for (size_t i=0 ; i<k ; i++) b->rec[b->serial[i]] = b->out[i];
		}
	free (items);
	select_device_of (chromsSorted[0]);
	const double t1 = now_ms ();

	size_t len = 0;
	for (u64 r=0 ; r<pending ; r++)
		{
		const row* w = &b->rows[r];
		const size_t chromLen = strlen (w->s->chrom);
		if (len + chromLen + 2200 > b->textCap)
			{
			if (len != 0) { fwrite (b->text, 1, len, f);  len = 0; }
			if (chromLen + 2200 > b->textCap)
				{
				b->textCap = (1u << 20) + chromLen + 2200;
				b->text = (char*) must_alloc (realloc (b->text, b->textCap), name);
				}
			}
		char* p = b->text + len;
		memcpy (p, w->s->chrom, chromLen);  p += chromLen;  *(p++) = '\t';
		p = put_unsigned (p, w->fileStart);  *(p++) = '\t';
		p = put_unsigned (p, w->fileEnd);
		p = put_interval_figures (p, &b->rec[r], w->s->start, op->originOne, op->sample.precision);
		len = (size_t) (p - b->text);
		}
	if (len != 0) fwrite (b->text, 1, len, f);
	op->msDevice += t1 - t0;  op->msFormat += now_ms () - t1;
	ib_begin ();                                               /* forget them */
	}

void op_statsover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_statsover* op = (dspop_statsover*) _op;
	char    line[1001], prevChrom[1001];
	char*   chrom;
	spec*   s = NULL;
	u32     start, end, o = op->originOne? 1 : 0;
	valtype val;
	batch   b;
	memset (&b, 0, sizeof(b));

	const double tStart = now_ms ();
	FILE* f = fopen (op->filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", _op->name, op->filename);  exit (EXIT_FAILURE); }
	FILE* out = open_table (_op->name, op->outFilename);
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;

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
			b.cap  = (b.cap == 0)? 4096 : 2*b.cap;
			b.rows = (row*) must_alloc (realloc (b.rows, b.cap * sizeof(row)), _op->name);
			b.rec  = (gdsp_interval_stat*) must_alloc (realloc (b.rec, b.cap * sizeof(gdsp_interval_stat)), _op->name);
			}
		b.rows[serial].s = s;  b.rows[serial].fileStart = fileStart;  b.rows[serial].fileEnd = end;
		ib_add (s, adjStart, adjEnd, (valtype) serial);
		op->bases += adjEnd - adjStart;
		if (ib_pending () >= ib_batch_limit ()) flush_batch (op, &b, ib_pending (), out);
		}
	fclose (f);
	flush_batch (op, &b, ib_pending (), out);
	close_table (out);
	if (getenv ("GDSP_STATSOVER_TIMES") != NULL)
		{
		const double all = now_ms () - tStart;
		fprintf (stderr, "[%s] times: %.1f ms = read and route %.1f + device calls %.1f + format and write %.1f\n", _op->name, all,
		         all - op->msDevice - op->msFormat, op->msDevice, op->msFormat);
		op->msDevice = op->msFormat = 0;
		}
	free (b.rows);  free (b.rec);  free (b.vec);  free (b.start);  free (b.end);  free (b.serial);  free (b.out);  free (b.text);
	}

/* the driver: the signal is only read, 8 B per base of the intervals' summed length since the last call */
static void statsover_work (dspop* op, u64* bases, double* bytesPerBase)
	{ *bases = ((dspop_statsover*) op)->bases;  ((dspop_statsover*) op)->bases = 0;  *bytesPerBase = 8; }

static const dspinfo statsoverRows[] =
	{ dspinforecord("statsover", op_statsover), dspinfoalias ("stats_over"), dspinfoalias ("intervalstats"),
	  dspinfoalias ("interval_stats") };
static const optraits statsoverTraits[] = { { op_statsover_apply, true, false, NULL, NULL, statsover_work } };
const opgroup opgroup_statsover = OPGROUP (statsoverRows, statsoverTraits, NULL);
