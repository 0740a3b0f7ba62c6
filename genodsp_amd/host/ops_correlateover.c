/* ops_correlateover.c -- correlateover (device shim).  Not an operator of the reference: a table with one line per interval of
 * a file -- correlate's figures of the signal against a second track over that interval alone: do two replicates agree
 * inside each peak, what are the treatment/control covariance and slope per gene or per bin, which promoters carry plus-
 * and minus-strand signal that moves together.  correlate (ops_correlate.c) reduces the genome to one line, and
 * localcorrelate (ops_localcorrelate.c) knows one fixed window around every base.  The signal is not modified and no
 * variable is set; the partners hold the track afterwards, as after correlate.
 *
 * The file of intervals is read, the intervals are batched and the lines are written by the half shared with statsover,
 * percentilesover and breadthover, which also takes the options they have in common (interval_table_run, interval_op:
 * ops_common.c; host_services.h says how).  The track is a second file, read once per run as `correlate <file>` reads it
 * (load_track_into_partners) into every chromosome's partner.  Each device then answers the intervals on its chromosomes
 * in one call (gdsp_interval_correlation_batch, include/genodsp_hip.h: every figure exact and rounded once or derived
 * from such, a function of the interval's sample alone).  What is this operator's own is that call, with each vector's
 * partner named as its track, the track's options, the header and the figures of a line.
 *
 * The driver finds this operator through opgroup_correlateover, at the end of this file (host_services.h); every call into
 * the device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_correlateover)

typedef struct dspop_correlateover
	{
	interval_op head;
	char*       trackFilename;
	int         valColumn;
	int         trackOriginOne;                 /* -1: what --origin resolves to */
	valtype     fileMin, fileMax;               /* --filemin / --filemax: the limits of the track's values */
	} dspop_correlateover;

OP_SHORT (op_correlateover, "print the correlation of the signal with a second track over each interval of a file (not in genodsp)")

void op_correlateover_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sPrint one line per interval of a file, in file order: chromosome, start, end, then over the\n", indent);
	fprintf (f, "%sbases of that interval the figures correlate gives for the genome: the count, the mean and\n", indent);
	fprintf (f, "%sstddev of the signal, filemean and filestddev of a second track (the values of the intervals\n", indent);
	fprintf (f, "%sin another file; bases under none are 0, overlapping intervals add up), their covariance,\n", indent);
	fprintf (f, "%scorrelation (Pearson r), and the slope and intercept of the track regressed on the signal.\n", indent);
	fprintf (f, "%sEach is exact and rounded once, or derived from such; what is not defined prints NA.\n", indent);
	fprintf (f, "%sIntervals may overlap and come in any order. The signal is not modified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> --track=<filename> [options]\n", indent, name);
	fprintf (f, "%s  --track=<file>           the second track's intervals (required)\n", indent);
	fprintf (f, "%s  --value=<col>            the track's values are in column <col> of its file\n", indent);
	fprintf (f, "%s  --novalue                the track's intervals have no value; every interval counts 1\n", indent);
	fprintf (f, "%s  --trackorigin=one|zero   coordinate convention of the track's file (default: --origin's)\n", indent);
	fprintf (f, "%s  --filemin=<value> --filemax=<value>  ignore bases whose track is outside this range\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout, when the operator runs)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore bases whose signal is outside this range\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        coordinate convention of the file of intervals\n", indent);
	}

dspop* op_correlateover_parse (char* name, int argc, char** argv)
	{
	dspop_correlateover* op = (dspop_correlateover*) new_op (name, sizeof(dspop_correlateover), true);
	interval_op_init (&op->head);
	op->valColumn      = (int) get_named_global ("valColumn", 4-1);
	op->trackOriginOne = -1;
	op->fileMin        = -valtypeMax;
	op->fileMax        =  valtypeMax;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (strcmp_prefix (arg, "--track=") == 0)
			{ if (op->trackFilename != NULL) free (op->trackFilename);  op->trackFilename = copy_string (argVal);  continue; }
		if (strcmp_prefix (arg, "--trackorigin=") == 0)
			{
			if      (strcmp (argVal, "one")  == 0) op->trackOriginOne = true;
			else if (strcmp (argVal, "zero") == 0) op->trackOriginOne = false;
			else chastise ("[%s] --trackorigin= takes one or zero (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--filemin=") == 0) { op->fileMin = string_to_valtype (argVal);  continue; }
		if (strcmp_prefix (arg, "--filemax=") == 0) { op->fileMax = string_to_valtype (argVal);  continue; }
		if (value_column_take (name, arg, &op->valColumn)) continue;
		interval_op_take (&op->head, name, arg);
		}
	interval_op_check (&op->head, name);
	if ((op->trackFilename == NULL) || (op->trackFilename[0] == 0)) chastise ("[%s] no track was provided (--track=<filename>)\n", name);
	if (op->fileMin > op->fileMax) chastise ("[%s] --filemin can't be above --filemax\n", name);
	if (op->trackOriginOne < 0) op->trackOriginOne = op->head.originOne;
	return (dspop*) op;
	}

void op_correlateover_free (dspop* _op)
	{
	dspop_correlateover* op = (dspop_correlateover*) _op;
	if (op->trackFilename != NULL) free (op->trackFilename);
	interval_op_free (&op->head);
	free (op);
	}

/* ------------------------------------------------------------------------------------- the table's figures ---- */
/* one device's share in one call: every vector's track is its chromosome's partner */
static void answer_correlation (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out)
	{
	dspop_correlateover* op = (dspop_correlateover*) ctx;
	char* name = op->head.common.name;
	for (int i=0 ; i<m ; i++)
		{
		spec* s = chromsOfInterest;
		while ((s != NULL) && (s->valVector != items[i].d_in)) s = s->next;
		if (s == NULL) { fprintf (stderr, "[%s] internal error: a vector that is no chromosome's\n", name);  exit (EXIT_FAILURE); }
		items[i].d_out = partner_of (s);
		}
	check_gdsp (gdsp_interval_correlation_batch (items, m, vec, start, end, k, op->head.sample.minAllowed, op->head.sample.maxAllowed,
	                                             op->fileMin, op->fileMax, (gdsp_interval_corr*) out, op_stream ()), name);
	}

/* a line: the name, two coordinates and the count (at most 20 digits each), eight figures of at most 400 characters, tabs */
#define correlation_line_max (100 + 401 * 8)

static char* put_correlation (void* ctx, char* p, const void* rec, arg_dont_complain(spec* s))
	{
	dspop_correlateover* op = (dspop_correlateover*) ctx;
	const gdsp_interval_corr* r = (const gdsp_interval_corr*) rec;
	const double fig[8] = { r->mean, r->filemean, r->stddev, r->filestddev, r->covariance, r->correlation, r->slope, r->intercept };
	*(p++) = '\t';
	p = put_unsigned (p, r->count);
	for (int j=0 ; j<8 ; j++)
		{
		*(p++) = '\t';
		if (fig[j] != fig[j]) { *(p++) = 'N';  *(p++) = 'A'; }
		else                  p = put_value (p, fig[j], op->head.sample.precision);
		}
	*(p++) = '\n';
	return p;
	}

static void put_header (arg_dont_complain(void* ctx), FILE* out)
	{ fputs ("#chrom\tstart\tend\tcount\tmean\tfilemean\tstddev\tfilestddev\tcovariance\tcorrelation\tslope\tintercept\n", out); }

void op_correlateover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_correlateover* op = (dspop_correlateover*) _op;
	to_whole ();                                               /* both files address whole chromosomes */
	load_track_into_partners (_op->name, op->trackFilename, op->valColumn, op->trackOriginOne);
	interval_table t = { sizeof(gdsp_interval_corr), answer_correlation, put_correlation, correlation_line_max, put_header, op, 0, 0, 0, 0 };
	interval_op_run (&op->head, &t);
	}

/* --report=gpu: two streams, two passes over the intervals' summed length */
static void correlateover_work (dspop* op, u64* bases, double* bytesPerBase)
	{
	interval_op_work (op, bases, bytesPerBase);
	*bytesPerBase = 32;
	}

static const dspinfo correlateoverRows[] =
	{ dspinforecord("correlateover", op_correlateover), dspinfoalias ("correlate_over"), dspinfoalias ("correlationover"),
	  dspinfoalias ("pearsonover") };
static const optraits correlateoverTraits[] = { { op_correlateover_apply, false, false, NULL, NULL, correlateover_work } };
const opgroup opgroup_correlateover = OPGROUP (correlateoverRows, correlateoverTraits, NULL);
