/* ops_lagcorr.c -- crosscorrelate, autocorrelate (device shim).  Not operators of the reference.  correlate compares the
 * signal with a second track base against the same base; these two ask at which shift two tracks agree best: the
 * covariance and correlation of the signal x against a track y shifted by every lag d of a range, y[i+d] against x[i].
 * For crosscorrelate y is a file of intervals, loaded into the partner buffers exactly as correlate loads its track
 * (load_track_into_partners of ops_correlate.c); for autocorrelate y is the signal itself and no partner is touched.
 * Plus-strand against minus-strand coverage gives the strand cross-correlation curve, whose peak is the fragment length;
 * the signal against itself shows nucleosome spacing and periodicity.
 *
 * The figures are gdsp_genome_lag_correlation's (include/genodsp_hip.h): per lag one exact sum of products rounded once,
 * divided by the size of lag 0's sample as R's acf / ccf do -- so what is printed does not depend on the number of
 * devices, the cut of the genome, chromosome order or the way the devices' images meet.  The signal is only read.
 *
 * The driver finds these operators through opgroup_lagcorr, at the end of this file (host_services.h); every call into the
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

dspprototypes(op_crosscorrelate)
dspprototypes(op_autocorrelate)

#define LAGCORR_MAX_LAGS 4096

typedef struct dspop_lagcorr
	{
	dspop common;
	int   withFile;                             /* crosscorrelate */
	char* filename;
	char* outFilename;
	int   valColumn, originOne, reportForBash, precision, quiet;
	int   haveLags, lagLo, lagHi;
	} dspop_lagcorr;

OP_SHORT (op_crosscorrelate, "covariance and correlation of the signal against the intervals in a file at every lag of a range (not in genodsp)")
OP_SHORT (op_autocorrelate,  "covariance and correlation of the signal against itself at every lag of a range (not in genodsp)")

static void lagcorr_usage_common (char* name, FILE* f, char* indent, int withFile)
	{
	fprintf (f, "%sEvery sum is exact and rounded once; each covariance is the sum of the lag's products\n", indent);
	fprintf (f, "%sdivided by the count of lag 0 (as R's acf and ccf divide), never across chromosomes.\n", indent);
	fprintf (f, "%sA table `lag pairs covariance correlation` is written, and the variables of correlate\n", indent);
	fprintf (f, "%s(from lag 0) and bestlag, bestcorrelation, mincorrelation are set. The signal is not\n", indent);
	fprintf (f, "%smodified. The work is bases x lags products: a genome at a few hundred lags takes on the\n", indent);
	fprintf (f, "%sorder of a second. Not in genodsp.\n\n", indent);
	if (withFile) fprintf (f, "%susage: %s <filename> --lags=<lo>..<hi> | --maxlag=<n> [options]\n", indent, name);
	else          fprintf (f, "%susage: %s --lags=<lo>..<hi> | --maxlag=<n> [options]\n", indent, name);
	fprintf (f, "%s  --lags=<lo>..<hi>        the lags to compute, at most %d of them\n", indent, LAGCORR_MAX_LAGS);
	if (withFile) fprintf (f, "%s  --maxlag=<n>             the same as --lags=-<n>..<n>\n", indent);
	else          fprintf (f, "%s  --maxlag=<n>             the same as --lags=0..<n>\n", indent);
	if (withFile)
		{
		fprintf (f, "%s  --value=<col>            intervals' values are in column <col> of the file\n", indent);
		fprintf (f, "%s  --novalue                intervals have no value; every interval counts 1\n", indent);
		fprintf (f, "%s  --origin=one|zero        intervals are origin-one, closed / origin-zero, half-open\n", indent);
		}
	fprintf (f, "%s  --output=<filename>      write the table to a file instead of stdout\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point when reporting (default: all of them)\n", indent);
	fprintf (f, "%s  --report:bash            print bestlag, bestcorrelation, mincorrelation as shell\n", indent);
	fprintf (f, "%s                           assignments on stdout\n", indent);
	fprintf (f, "%s  --quiet                  do not report those three on stderr\n", indent);
	}

void op_crosscorrelate_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sShift a second track, the values of the intervals in a file (bases under no interval\n", indent);
	fprintf (f, "%sare 0, overlapping intervals add up), against the signal: for every lag d of a range, the\n", indent);
	fprintf (f, "%scovariance and correlation of signal[i] with track[i+d] (strand cross-correlation).\n", indent);
	lagcorr_usage_common (name, f, indent, true);
	}

void op_autocorrelate_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sShift the signal against itself: for every lag d of a range, the covariance and\n", indent);
	fprintf (f, "%scorrelation of signal[i] with signal[i+d] (periodicity, nucleosome spacing).\n", indent);
	lagcorr_usage_common (name, f, indent, false);
	}

static dspop* lagcorr_parse (char* name, int argc, char** argv, int withFile)
	{
	dspop_lagcorr* op = (dspop_lagcorr*) new_op (name, sizeof(dspop_lagcorr), true);
	op->withFile  = withFile;
	op->valColumn = (int) get_named_global ("valColumn", 4-1);
	op->originOne = (int) get_named_global ("originOne", false);
	op->precision = -1;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (strcmp_prefix (arg, "--lags=") == 0)
			{
			char* dots = strstr (argVal, "..");
			if ((dots == NULL) || (dots == argVal) || (dots[2] == 0))
				chastise ("[%s] the lags are given as <lo>..<hi> (\"%s\")\n", name, arg);
			char* lo = copy_string (argVal);
			lo[dots - argVal] = 0;
			op->lagLo = string_to_int (lo);
			op->lagHi = string_to_int (dots + 2);
			free (lo);
			if (op->lagLo > op->lagHi) chastise ("[%s] the first lag can't be above the last (\"%s\")\n", name, arg);
			op->haveLags = true;
			continue;
			}
		if (strcmp_prefix (arg, "--maxlag=") == 0)
			{
			int n = string_to_int (argVal);
			if (n < 0) chastise ("[%s] the largest lag can't be negative (\"%s\")\n", name, arg);
			op->lagLo = withFile? -n : 0;
			op->lagHi = n;
			op->haveLags = true;
			continue;
			}
		if (is_opt3 (arg, "window", "W") || (strcmp_prefix (arg, "--min=") == 0) || (strcmp_prefix (arg, "--max=") == 0))
			chastise ("[%s] every base of every chromosome is looked at: no window and no limits (\"%s\")\n", name, arg);
		if (strcmp_prefix (arg, "--precision=") == 0)
			{
			op->precision = string_to_int (argVal);
			if (op->precision < 0) chastise ("[%s] precision can't be negative (\"%s\")\n", name, arg);
			continue;
			}
		if ((strcmp (arg, "--quiet") == 0) || (strcmp (arg, "--silent") == 0)) { op->quiet = true;  continue; }
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if ((strcmp (arg, "--report:bash") == 0) || (strcmp (arg, "--bash") == 0)) { op->reportForBash = true;  continue; }
		if (withFile && value_column_take (name, arg, &op->valColumn)) continue;
		if (withFile && origin_opt_take (arg, &op->originOne)) continue;
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (withFile && (op->filename == NULL)) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (withFile && (op->filename == NULL)) chastise ("[%s] no filename was provided\n", name);
	if (!op->haveLags) chastise ("[%s] no lag range was provided (--lags=<lo>..<hi> or --maxlag=<n>)\n", name);
	if ((long long) op->lagHi - op->lagLo + 1 > LAGCORR_MAX_LAGS)
		chastise ("[%s] at most %d lags can be computed at once (%d..%d)\n", name, LAGCORR_MAX_LAGS, op->lagLo, op->lagHi);
	if (op->reportForBash && op->quiet) chastise ("[%s] Can't use both --report:bash and --quiet\n", name);
	return (dspop*) op;
	}

dspop* op_crosscorrelate_parse (char* name, int argc, char** argv) { return lagcorr_parse (name, argc, argv, true); }
dspop* op_autocorrelate_parse  (char* name, int argc, char** argv) { return lagcorr_parse (name, argc, argv, false); }

static void lagcorr_free (dspop* _op)
	{
	dspop_lagcorr* op = (dspop_lagcorr*) _op;
	if (op->filename    != NULL) free (op->filename);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

void op_crosscorrelate_free (dspop* op) { lagcorr_free (op); }
void op_autocorrelate_free  (dspop* op) { lagcorr_free (op); }

static void lagcorr_apply (dspop* _op)
	{
	dspop_lagcorr* op = (dspop_lagcorr*) _op;
	char* name = _op->name;
	const u32 nlags = (u32) (op->lagHi - op->lagLo + 1);
	to_whole ();                                               /* lagged pairs are pairs of one whole chromosome */
	if (op->withFile) load_track_into_partners (name, op->filename, op->valColumn, op->originOne);

	sigpart* parts;
	int npairs = signal_parts (&parts);
	gdsp_xsum_pair* pairs = (gdsp_xsum_pair*) calloc (npairs? npairs : 1, sizeof(gdsp_xsum_pair));
	uint64_t* count = (uint64_t*) calloc (nlags, sizeof(uint64_t));
	double*   cov   = (double*)   calloc (2 * (size_t) nlags, sizeof(double));
	if ((pairs == NULL) || (count == NULL) || (cov == NULL)) { fprintf (stderr, "[%s] out of memory\n", name);  exit (EXIT_FAILURE); }
	double* corr = cov + nlags;
	sync_all_devices ();                                       /* (the track is in place everywhere) */
	for (int i=0 ; i<npairs ; i++)
		{
		select_device_of (parts[i].s);
		pairs[i].d_x = parts[i].v;
		pairs[i].d_y = op->withFile? partner_of (parts[i].s) + (parts[i].v - parts[i].s->valVector) : parts[i].v;
		pairs[i].n = parts[i].n;  pairs[i].first = parts[i].first;
		pairs[i].device = physical_device_of (parts[i].s);  pairs[i].stream = op_stream ();
		}
	if (npairs > 0) select_device_of (parts[0].s);
	void* reduceCtx = NULL;
	gdsp_reduce_fn reduce = reduce_over_devices (&reduceCtx);      /* (also hands the communicator to the library) */
	double fig[GDSP_CORR_FIGURES];
	check_gdsp (gdsp_genome_lag_correlation (pairs, npairs, op->lagLo, nlags, reduce, reduceCtx, fig, count, cov, corr), name);
	free (pairs);

	/* the table */
	FILE* out = open_table (name, op->outFilename);
	char  a[400], b[400];
	const int haveSample = fig[GDSP_CORR_COUNT] != 0;
	format_value (a, sizeof(a), fig[GDSP_CORR_COUNT], op->precision);
	fprintf (out, "# count %s\n", a);
	format_value (a, sizeof(a), fig[GDSP_CORR_MEANX], op->precision);  format_value (b, sizeof(b), fig[GDSP_CORR_SDX], op->precision);
	fprintf (out, "# mean %s\n# stddev %s\n", a, b);
	if (op->withFile)
		{
		format_value (a, sizeof(a), fig[GDSP_CORR_MEANY], op->precision);  format_value (b, sizeof(b), fig[GDSP_CORR_SDY], op->precision);
		fprintf (out, "# filemean %s\n# filestddev %s\n", a, b);
		}
	fprintf (out, "#lag\tpairs\tcovariance\tcorrelation\n");
	int    haveBest = false, bestLag = 0;
	double bestCorr = 0, minCorr = 0;
	for (u32 k=0 ; k<nlags ; k++)
		{
		const int d = op->lagLo + (int) k;
		format_value (a, sizeof(a), cov[k], op->precision);  format_value (b, sizeof(b), corr[k], op->precision);
		fprintf (out, "%d\t%llu\t%s\t%s\n", d, (unsigned long long) count[k], a, b);
		if (isnan (corr[k])) continue;
		/* the largest correlation; ties go to the smaller |lag|, then to the smaller lag (which is met first) */
		if (!haveBest || (corr[k] > bestCorr) || ((corr[k] == bestCorr) && (abs (d) < abs (bestLag))))
			{ bestCorr = corr[k];  bestLag = d; }
		if (!haveBest || (corr[k] < minCorr)) minCorr = corr[k];
		haveBest = true;
		}
	close_table (out);

	/* correlate's variables, from lag 0's sample (which is every lag's) */
	static const struct { char* name;  int k; } vars[] =
		{ { "count", GDSP_CORR_COUNT }, { "mean", GDSP_CORR_MEANX }, { "variance", GDSP_CORR_VARX }, { "stddev", GDSP_CORR_SDX },
		  { "filemean", GDSP_CORR_MEANY }, { "filevariance", GDSP_CORR_VARY }, { "filestddev", GDSP_CORR_SDY },
		  { "covariance", GDSP_CORR_COV }, { "correlation", GDSP_CORR_CORRELATION }, { "slope", GDSP_CORR_SLOPE },
		  { "intercept", GDSP_CORR_INTERCEPT } };
	for (size_t k=0 ; k<sizeof(vars)/sizeof(vars[0]) ; k++)
		{ if (haveSample || (k == 0)) set_named_global (vars[k].name, fig[vars[k].k]); }
	if (haveBest)
		{
		const struct { char* name;  double x; } best[3] =
			{ { "bestlag", (double) bestLag }, { "bestcorrelation", bestCorr }, { "mincorrelation", minCorr } };
		for (int k=0 ; k<3 ; k++)
			{
			set_named_global (best[k].name, best[k].x);
			if (op->quiet) continue;
			format_value (a, sizeof(a), best[k].x, op->precision);
			if (op->reportForBash) fprintf (stdout, "%s=%s # bash command\n", best[k].name, a);
			else                   fprintf (stderr, "%s is %s\n", best[k].name, a);
			}
		}
	else if (!haveSample)
		fprintf (stderr, "[%s] nothing can be computed;  no base has a finite value in both tracks\n", name);
	else
		fprintf (stderr, "[%s] no lag has a correlation;  a track is constant, or its products overflow\n", name);
	free (count);  free (cov);
	}

void op_crosscorrelate_apply (dspop* op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{ lagcorr_apply (op); }

void op_autocorrelate_apply (dspop* op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{ lagcorr_apply (op); }

/* the driver: autocorrelate is the signal against itself, no partner is touched */
static const dspinfo lagcorrRows[] =
	{ dspinforecord("crosscorrelate", op_crosscorrelate), dspinfoalias ("cross_correlate"), dspinfoalias ("xcorr"), dspinfoalias ("ccf"),
	  dspinforecord("autocorrelate" , op_autocorrelate) , dspinfoalias ("autocorrelation"), dspinfoalias ("acf") };
static const optraits lagcorrTraits[] = { { op_autocorrelate_apply, true, false, NULL, NULL, NULL } };
const opgroup opgroup_lagcorr = OPGROUP (lagcorrRows, lagcorrTraits, gdsp_genome_lag_correlation_use_comm);
