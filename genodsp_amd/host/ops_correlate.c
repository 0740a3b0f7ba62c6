/* ops_correlate.c -- correlate (device shim).  Not an operator of the reference, which can only fold a second track
 * into the signal (add, subtract, multiply, divide <file>): how alike are the signal and another track -- treatment and
 * control, two replicates, before and after smooth -- and by what factor does one sit on the other's scale.
 *
 * The track is a file of intervals read by the rules of `add <file>` (read_interval, the value column and origin of the
 * command line, the same complaint about an interval beyond the chromosome's end).  y is what `add <file>` would leave
 * on an all-zero genome: bases under no interval are 0, overlapping intervals sum in file order, unknown chromosomes
 * are ignored.  It is built in each chromosome's partner buffer, which is nobody's data between operators; the signal
 * is only read.  The figures are gdsp_genome_correlation's (include/genodsp_hip.h): exact sums rounded once, and the
 * correlation, slope and intercept derived from them -- so what is printed does not depend on the number of devices,
 * the cut of the genome, chromosome order, the interval batches or the way the devices' images meet.
 *
 * The driver finds this operator through opgroup_correlate, at the end of this file (host_services.h); every call into the
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

dspprototypes(op_correlate)

typedef struct dspop_correlate
	{
	dspop       common;
	sample_opts sample;                         /* (as stats: window, --min / --max of the signal, precision, quiet) */
	char*       filename;
	int         valColumn, originOne, reportForBash;
	valtype     fileMin, fileMax;               /* --filemin / --filemax: the limits of the track's values */
	} dspop_correlate;

OP_SHORT (op_correlate, "covariance, Pearson correlation and regression of the signal against the intervals in a file (not in genodsp)")

void op_correlate_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sCompare the signal with a second track, the values of the intervals in a file (bases\n", indent);
	fprintf (f, "%sunder no interval are 0, overlapping intervals add up): the count, mean, variance and\n", indent);
	fprintf (f, "%sstddev of the signal, filemean, filevariance and filestddev of the track, and their\n", indent);
	fprintf (f, "%scovariance, correlation (Pearson r), and the slope and intercept of the track regressed\n", indent);
	fprintf (f, "%son the signal. Each is exact and rounded once, or derived from such, and is stored in a\n", indent);
	fprintf (f, "%snamed variable. The signal is not modified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> [options]\n", indent, name);
	fprintf (f, "%s  --value=<col>            intervals' values are in column <col> of the file\n", indent);
	fprintf (f, "%s  --novalue                intervals have no value; every interval counts 1\n", indent);
	fprintf (f, "%s  --origin=one|zero        intervals are origin-one, closed / origin-zero, half-open\n", indent);
	fprintf (f, "%s  --window=<length>        (W=) look at one base per window\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>          ignore bases whose signal is outside this range\n", indent);
	fprintf (f, "%s  --filemin=<value> --filemax=<value>  ignore bases whose track is outside this range\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point when reporting (default: all of them)\n", indent);
	fprintf (f, "%s  --report:bash            print results as shell assignments on stdout\n", indent);
	fprintf (f, "%s  --quiet                  do not report results on stderr\n", indent);
	}

dspop* op_correlate_parse (char* name, int argc, char** argv)
	{
	dspop_correlate* op = (dspop_correlate*) new_op (name, sizeof(dspop_correlate), true);
	sample_opts_init (&op->sample);
	op->valColumn = (int) get_named_global ("valColumn", 4-1);
	op->originOne = (int) get_named_global ("originOne", false);
	op->fileMin   = -valtypeMax;
	op->fileMax   =  valtypeMax;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (sample_opts_take (&op->sample, name, arg, SAMPLE_OPT_WINDOW | SAMPLE_OPT_QUIET | SAMPLE_OPT_PRECISION)) continue;
		if (strcmp_prefix (arg, "--filemin=") == 0) { op->fileMin = string_to_valtype (argVal);  continue; }
		if (strcmp_prefix (arg, "--filemax=") == 0) { op->fileMax = string_to_valtype (argVal);  continue; }
		if (value_column_take (name, arg, &op->valColumn)) continue;
		if (origin_opt_take (arg, &op->originOne)) continue;
		if ((strcmp (arg, "--report:bash") == 0) || (strcmp (arg, "--bash") == 0)) { op->reportForBash = true;  continue; }
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (op->filename == NULL) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->filename == NULL) chastise ("[%s] no filename was provided\n", name);
	if (op->reportForBash && op->sample.quiet) chastise ("[%s] Can't use both --report:bash and --quiet\n", name);
	return (dspop*) op;
	}

void op_correlate_free (dspop* _op)
	{
	dspop_correlate* op = (dspop_correlate*) _op;
	if (op->filename != NULL) free (op->filename);
	free (op);
	}

/* y, into every chromosome's partner: what `add <file>` (ops_intervals.c) would leave on zeros.  The first batch starts
 * every base of every chromosome from 0, the later ones add to what is there, as the main ingest does */
void load_track_into_partners (char* name, char* filename, int valColumn, int originOne)
	{
	char    line[1001], prevChrom[1001];
	char*   chrom;
	spec*   s = NULL;
	u32     start, end, o = originOne? 1 : 0;
	valtype val;
	int     clearFlags = GDSP_CLEAR_FILL;

	FILE* f = fopen (filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", name, filename);  exit (EXIT_FAILURE); }
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;
	ib_begin ();
	prevChrom[0] = 0;
	while (read_interval (f, line, sizeof(line), valColumn, &chrom, &start, &end, &val))
		{
		if (val == 0.0) continue;                              /* (as add: add.c:235) */
		if (strcmp (chrom, prevChrom) != 0)
			{ s = find_chromosome_spec (chrom);  safe_strncpy (prevChrom, chrom, sizeof(prevChrom)-1); }
		if (s == NULL) continue;
		if (!s->flag) { if (trackOperations) fprintf (stderr, "%s(%s)\n", name, chrom);  s->flag = true; }
		start -= o;
		u32 adjStart, adjEnd;
		if (!place_interval (name, filename, chrom, s, start, end, &adjStart, &adjEnd)) continue;
		ib_add (s, adjStart, adjEnd, val);
		if (ib_pending () >= ib_batch_limit ())
			{
			ib_flush_apply_partner (ri_overlapSum, clearFlags, 0.0, clearFlags != 0);
			clearFlags = 0;
			}
		}
	fclose (f);
	ib_flush_apply_partner (ri_overlapSum, clearFlags, 0.0, clearFlags != 0);
	}

void op_correlate_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_correlate* op = (dspop_correlate*) _op;
	char* name = _op->name;
	to_whole ();                                               /* the file addresses whole chromosomes */
	load_track_into_partners (name, op->filename, op->valColumn, op->originOne);

	/* the signal's parts, each with the partner at the same offset */
	sigpart* parts;
	int npairs = signal_parts (&parts);
	gdsp_xsum_pair* pairs = (gdsp_xsum_pair*) calloc (npairs? npairs : 1, sizeof(gdsp_xsum_pair));
	if (pairs == NULL) { fprintf (stderr, "[%s] out of memory\n", name);  exit (EXIT_FAILURE); }
	sync_all_devices ();                                       /* (the track is in place everywhere) */
	for (int i=0 ; i<npairs ; i++)
		{
		select_device_of (parts[i].s);
		pairs[i].d_x = parts[i].v;  pairs[i].d_y = partner_of (parts[i].s) + (parts[i].v - parts[i].s->valVector);
		pairs[i].n = parts[i].n;  pairs[i].first = parts[i].first;
		pairs[i].device = physical_device_of (parts[i].s);  pairs[i].stream = op_stream ();
		}
	if (npairs > 0) select_device_of (parts[0].s);
	void* reduceCtx = NULL;
	gdsp_reduce_fn reduce = reduce_over_devices (&reduceCtx);      /* (also hands the communicator to the library) */
	double fig[GDSP_CORR_FIGURES];
	check_gdsp (gdsp_genome_correlation (pairs, npairs, op->sample.window, op->sample.minAllowed, op->sample.maxAllowed,
	                                     op->fileMin, op->fileMax, reduce, reduceCtx, fig), name);
	free (pairs);

	static const struct { char* name;  int k; } vars[] =
		{ { "count", GDSP_CORR_COUNT }, { "mean", GDSP_CORR_MEANX }, { "variance", GDSP_CORR_VARX }, { "stddev", GDSP_CORR_SDX },
		  { "filemean", GDSP_CORR_MEANY }, { "filevariance", GDSP_CORR_VARY }, { "filestddev", GDSP_CORR_SDY },
		  { "covariance", GDSP_CORR_COV }, { "correlation", GDSP_CORR_CORRELATION }, { "slope", GDSP_CORR_SLOPE },
		  { "intercept", GDSP_CORR_INTERCEPT } };
	for (size_t k=0 ; k<sizeof(vars)/sizeof(vars[0]) ; k++)
		{
		const double x = fig[vars[k].k];
		if ((fig[GDSP_CORR_COUNT] == 0) && (k >= 1)) continue;   /* (no mean of nothing) */
		set_named_global (vars[k].name, x);
		if (op->sample.quiet) continue;
		char text[400];
		format_value (text, sizeof(text), x, op->sample.precision);
		if (op->reportForBash) fprintf (stdout, "%s=%s # bash command\n", vars[k].name, text);
		else                   fprintf (stderr, "%s is %s\n", vars[k].name, text);
		}
	if (fig[GDSP_CORR_COUNT] == 0)
		fprintf (stderr, "[%s] nothing can be computed;  no input values meet the criteria\n", name);
	}

/* the driver: no traits of its own (the track is built in the partners; it is a file-driven operator on whole chromosomes) */
static const dspinfo correlateRows[] =
	{ dspinforecord("correlate", op_correlate), dspinfoalias ("correlation"), dspinfoalias ("pearson"), dspinfoalias ("covariance") };
const opgroup opgroup_correlate = { correlateRows, (int) (sizeof(correlateRows)/sizeof(correlateRows[0])), NULL, 0, gdsp_genome_correlation_use_comm };
