/* ops_histogram.c -- histogram (device shim).  Not an operator of the reference: the genome-wide distribution of the
 * signal -- how many bases sit in each bin of an edge table, and the share of the genome at or above each bin's lower
 * edge (breadth of coverage at depth >= N), the table bedtools genomecov and mosdepth's dist file print.
 *
 * A whole-genome operator like stats: it samples the signal by stats' rules (--window counted from each chromosome's
 * first base, --min / --max, finite values only) wherever it lives -- whole chromosomes or, under --sharding=bases, the
 * stretches each device answers for -- and counts in one read of it (gdsp_genome_histogram, include/genodsp_hip.h).  The
 * counts are integers, so the table does not depend on the number of devices, the cut of the genome, chromosome order or
 * the way the devices' words meet (RCCL all-reduce of u64 words, or a host sum with --reduce=host).  The signal is not
 * modified; the variables count and mode are set.
 *
 * The driver finds this operator through opgroup_histogram, at the end of this file (host_services.h); every call into the
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

dspprototypes(op_histogram)

#define HISTOGRAM_MAX_BINS 65536

typedef struct dspop_histogram
	{
	dspop       common;
	sample_opts sample;                         /* (as stats) */
	u32         numBins;
	double*     edges;                          /* numBins + 1 of them */
	int         uniform;                        /* the table is lo + k*width */
	char*       outFilename;
	} dspop_histogram;

OP_SHORT (op_histogram, "print the genome-wide distribution of the values: count, fraction and breadth per bin (not in genodsp)")

void op_histogram_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sPrint how many bases of the genome fall into each bin of a table of values: one line per\n", indent);
	fprintf (f, "%sbin with its edges (lo <= value < hi), its count, its fraction of the counted bases and the\n", indent);
	fprintf (f, "%sfraction at or above its lower edge (breadth of coverage). Every count is exact. Sets the\n", indent);
	fprintf (f, "%svariables count and mode (lower edge of the fullest bin). The signal is not modified.\n", indent);
	fprintf (f, "%sNot in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s [options]\n", indent, name);
	fprintf (f, "%s  --bins=<number>          number of uniform bins, 1..65536 (default: 256)\n", indent);
	fprintf (f, "%s  --lo=<value>             lower edge of the first bin (default: 0)\n", indent);
	fprintf (f, "%s  --width=<value>          width of a bin (default: 1)\n", indent);
	fprintf (f, "%s  --edges=<file>           bin edges from a file instead, one per line, increasing (2..65537)\n", indent);
	fprintf (f, "%s  --window=<length>        (W=) look at one base per window\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout, when the operator runs)\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point of the edges (default: all of them)\n", indent);
	fprintf (f, "%s  --quiet                  do not report count and mode on stderr\n", indent);
	}

/* the edges of a file: one number per line, # comments and blank lines skipped; complaints end the run with the usage */
static double* read_edges (char* name, char* filename, u32* numBins)
	{
	FILE* f = fopen (filename, "rt");
	if (f == NULL) chastise ("[%s] can't open \"%s\" for reading\n", name, filename);
	double* e = (double*) malloc ((HISTOGRAM_MAX_BINS + 1) * sizeof(double));
	if (e == NULL) { fprintf (stderr, "[%s] out of memory\n", name);  exit (EXIT_FAILURE); }
	char line[1001];
	u32  n = 0, lineNum = 0;
	while (fgets (line, sizeof(line), f) != NULL)
		{
		lineNum++;
		char* hash = strchr (line, '#');  if (hash != NULL) *hash = 0;
		char* s = line;
		while ((*s == ' ') || (*s == '\t')) s++;
		size_t len = strlen (s);
		while ((len > 0) && ((s[len-1] == '\n') || (s[len-1] == '\r') || (s[len-1] == ' ') || (s[len-1] == '\t'))) s[--len] = 0;
		if (len == 0) continue;
		double v;
		if (!try_string_to_double (s, &v) || !(fabs (v) <= DBL_MAX))
			{ fclose (f);  chastise ("[%s] \"%s\" line %u: \"%s\" is not a finite number\n", name, filename, lineNum, s); }
		if (n > HISTOGRAM_MAX_BINS)
			{ fclose (f);  chastise ("[%s] \"%s\" holds more than %d edges\n", name, filename, HISTOGRAM_MAX_BINS + 1); }
		if ((n > 0) && !(e[n-1] < v))
			{ fclose (f);  chastise ("[%s] \"%s\" line %u: the edges must be strictly increasing (\"%s\")\n", name, filename, lineNum, s); }
		e[n++] = v;
		}
	fclose (f);
	if (n < 2) chastise ("[%s] \"%s\" holds fewer than 2 edges\n", name, filename);
	*numBins = n - 1;
	return e;
	}

dspop* op_histogram_parse (char* name, int argc, char** argv)
	{
	dspop_histogram* op = (dspop_histogram*) new_op (name, sizeof(dspop_histogram), true);
	sample_opts_init (&op->sample);
	int    bins = 256, haveUniform = false;
	double lo = 0, width = 1;
	char*  edgesFilename = NULL;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (sample_opts_take (&op->sample, name, arg, SAMPLE_OPT_WINDOW | SAMPLE_OPT_PRECISION | SAMPLE_OPT_QUIET)) continue;
		if (strcmp_prefix (arg, "--bins=") == 0)
			{
			bins = string_to_int (argVal);
			if ((bins < 1) || (bins > HISTOGRAM_MAX_BINS)) chastise ("[%s] the number of bins must be 1..%d (\"%s\")\n", name, HISTOGRAM_MAX_BINS, arg);
			haveUniform = true;
			continue;
			}
		if (strcmp_prefix (arg, "--lo=") == 0) { lo = string_to_double (argVal);  haveUniform = true;  continue; }
		if (strcmp_prefix (arg, "--width=") == 0)
			{
			width = string_to_double (argVal);
			if (!(width > 0)) chastise ("[%s] the bin width must be positive (\"%s\")\n", name, arg);
			haveUniform = true;
			continue;
			}
		if (strcmp_prefix (arg, "--edges=") == 0)
			{ if (edgesFilename != NULL) free (edgesFilename);  edgesFilename = copy_string (argVal);  continue; }
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if ((edgesFilename != NULL) && haveUniform)
		chastise ("[%s] Can't use --edges with --bins, --lo or --width\n", name);
	if (edgesFilename != NULL)
		{
		op->edges = read_edges (name, edgesFilename, &op->numBins);
		free (edgesFilename);
		}
	else
		{
		op->numBins = (u32) bins;
		op->uniform = true;
		op->edges   = (double*) malloc ((op->numBins + 1) * sizeof(double));
		if (op->edges == NULL) { fprintf (stderr, "[%s] out of memory\n", name);  exit (EXIT_FAILURE); }
		if (gdsp_histogram_uniform_edges (lo, width, op->numBins, op->edges) != GDSP_OK)      /* (host code: no device is touched) */
			chastise ("[%s] --lo=%.17g --width=%.17g --bins=%d do not give strictly increasing finite edges\n", name, lo, width, bins);
		}
	return (dspop*) op;
	}

void op_histogram_free (dspop* _op)
	{
	dspop_histogram* op = (dspop_histogram*) _op;
	if (op->edges       != NULL) free (op->edges);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

void op_histogram_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_histogram* op = (dspop_histogram*) _op;
	const u32 B = op->numBins;
	gdsp_xsum_source* src;
	int nsrc = signal_sources (_op->name, &src);
	u64* words = (u64*) calloc ((size_t) B + 3, sizeof(u64));
	if (words == NULL) { fprintf (stderr, "[%s] out of memory\n", _op->name);  exit (EXIT_FAILURE); }
	void* reduceCtx = NULL;
	gdsp_reduce_fn reduce = reduce_over_devices (&reduceCtx);    /* (NULL when the library's communicator does it) */
	check_gdsp (gdsp_genome_histogram (src, nsrc, op->sample.window, op->sample.minAllowed, op->sample.maxAllowed, op->edges, B,
	                                   op->uniform, reduce, reduceCtx, (uint64_t*) words), _op->name);
	free (src);

	const u64 below = words[B], above = words[B+1], n = words[B+2];
	FILE* out = open_table (_op->name, op->outFilename);
	char  lo[400], hi[400], text[400];
	fprintf (out, "# count %llu\n# below %llu\n# above %llu\n", (unsigned long long) n, (unsigned long long) below, (unsigned long long) above);
	fprintf (out, "#lo\thi\tcount\tfraction\tatleast\n");
	u64 atLeast = n - below;                                     /* sampled values at or above the bin's lower edge */
	u32 mode = 0;
	for (u32 k=0 ; k<B ; k++)
		{
		format_value (lo, sizeof(lo), op->edges[k],   op->sample.precision);
		format_value (hi, sizeof(hi), op->edges[k+1], op->sample.precision);
		fprintf (out, "%s\t%s\t%llu\t", lo, hi, (unsigned long long) words[k]);
		if (n == 0) fprintf (out, "NA\tNA\n");
		else        fprintf (out, "%.17g\t%.17g\n", (double) words[k] / (double) n, (double) atLeast / (double) n);
		atLeast -= words[k];
		if (words[k] > words[mode]) mode = k;                      /* (the lowest bin on ties) */
		}
	close_table (out);

	/* count as stats sets and words it; mode only when some bin holds something */
	set_named_global ("count", (valtype) n);
	if (!op->sample.quiet)
		{
		format_value (text, sizeof(text), (double) n, op->sample.precision);
		fprintf (stderr, "count is %s\n", text);
		}
	if (n - below - above != 0)
		{
		set_named_global ("mode", (valtype) op->edges[mode]);
		if (!op->sample.quiet)
			{
			format_value (text, sizeof(text), op->edges[mode], op->sample.precision);
			fprintf (stderr, "mode is %s\n", text);
			}
		}
	free (words);
	}

/* the driver: one read of the signal's parts as they are, each with its `first` */
static void histogram_work (dspop* op, u64* bases, double* bytesPerBase) { *bytesPerBase = 8; }

static const dspinfo  histogramRows[]   = { dspinforecord("histogram", op_histogram), dspinfoalias ("hist"), dspinfoalias ("distribution") };
static const optraits histogramTraits[] = { { op_histogram_apply, true, true, NULL, NULL, histogram_work } };
const opgroup opgroup_histogram = OPGROUP (histogramRows, histogramTraits, gdsp_genome_histogram_use_comm);
