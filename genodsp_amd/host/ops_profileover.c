/* ops_profileover.c -- profileover (device shim).  Not an operator of the reference: what the signal looks like, on
 * average, around the positions a file names -- read depth from 2 kb before to 2 kb behind every transcription start,
 * oriented by strand; the footprint around a million motif sites (the aggregate profile, or metaplot, of deepTools'
 * computeMatrix + plotProfile).  One table line per column of offsets: count, sum, mean, stddev and stderr of the values
 * found that far from the anchors, in each anchor's own direction.  The signal is not modified.
 *
 * The file is read and routed as statsover reads its own (origin, chromosomes the run does not hold are skipped, the trace
 * lines), but by a reader of its own (read_anchor_file, ops_common.c: matrixover shares it), which also fetches the strand
 * column; read_interval is left as it is.  Each
 * interval gives one anchor, from the interval as the file has it and before any clipping; an anchor that does not lie
 * in its chromosome's vector is skipped and counted.  The anchors stay on the host, 8 bytes each, for both passes.
 *
 * The figures are gdsp_genome_profile's (include/genodsp_hip.h): per column the exact sums rounded once, functions of the
 * column's sample alone -- so what is printed does not depend on the number of devices, on the cut of the genome, on
 * chromosome order or on the order of the file's lines.
 *
 * The driver finds this operator through opgroup_profileover, at the end of this file (host_services.h); every call into
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

dspprototypes(op_profileover)

typedef struct dspop_profileover
	{
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                         /* (its limits, precision and quiet; no window) */
	anchor_opts where;                          /* the anchors and the offsets around them (host_services.h) */
	int         reportForBash;
	u64         pairs;                          /* anchors times offsets of the last call (--report=gpu) */
	} dspop_profileover;

OP_SHORT (op_profileover, "print the exact average signal at every offset around the anchors a file names (not in genodsp)")

void op_profileover_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sThe aggregate profile (metaplot) of the signal around the positions a file names: every\n", indent);
	fprintf (f, "%sinterval of the file gives one anchor, and for every offset of a range the values found that\n", indent);
	fprintf (f, "%sfar from the anchors -- downstream is the anchor's own direction when a strand column is\n", indent);
	fprintf (f, "%snamed -- are counted, summed and averaged; every sum is exact and rounded once. One line per\n", indent);
	fprintf (f, "%scolumn of offsets is written: lo hi count sum mean stddev stderr (hi exclusive; NA where\n", indent);
	fprintf (f, "%snothing was found). A window that leaves its chromosome contributes the offsets that stay\n", indent);
	fprintf (f, "%sinside. The variables anchors, bestoffset and bestmean are set. The signal is not modified.\n", indent);
	fprintf (f, "%sNot in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> --flank=<bases> | --upstream=<bases> --downstream=<bases> [options]\n", indent, name);
	fprintf (f, "%s  --flank=<bases>          offsets -<bases> .. <bases>\n", indent);
	fprintf (f, "%s  --upstream=<bases> --downstream=<bases>  offsets -<upstream> .. <downstream>, at most %d\n", indent, GDSP_PROFILE_MAX_OFFSETS);
	fprintf (f, "%s  --anchor=start|end|center  where in its interval the anchor lies, in the interval's own\n", indent);
	fprintf (f, "%s                           direction (default: start)\n", indent);
	fprintf (f, "%s  --strand=<col>           column <col> of the file holds the strand; a field that begins\n", indent);
	fprintf (f, "%s                           with - is the minus strand (default: every anchor is plus)\n", indent);
	fprintf (f, "%s  --bin=<bases>            offsets per column; must divide their number (default: 1)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout)\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        intervals are origin-one, closed / origin-zero, half-open\n", indent);
	fprintf (f, "%s  --report:bash            print bestoffset and bestmean as shell assignments on stdout\n", indent);
	fprintf (f, "%s  --quiet                  do not report those two on stderr\n", indent);
	}

dspop* op_profileover_parse (char* name, int argc, char** argv)
	{
	dspop_profileover* op = (dspop_profileover*) new_op (name, sizeof(dspop_profileover), true);
	sample_opts_init (&op->sample);
	anchor_opts_init (&op->where);
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (anchor_opts_take (&op->where, name, arg)) continue;
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if ((strcmp (arg, "--report:bash") == 0) || (strcmp (arg, "--bash") == 0)) { op->reportForBash = true;  continue; }
		if (sample_opts_take (&op->sample, name, arg, SAMPLE_OPT_PRECISION | SAMPLE_OPT_QUIET)) continue;
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (op->filename == NULL) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->filename == NULL) chastise ("[%s] no filename was provided\n", name);
	anchor_opts_check (&op->where, name);
	if (op->sample.minAllowed > op->sample.maxAllowed) chastise ("[%s] --min can't be above --max\n", name);
	if (op->reportForBash && op->sample.quiet) chastise ("[%s] Can't use both --report:bash and --quiet\n", name);
	return (dspop*) op;
	}

void op_profileover_free (dspop* _op)
	{
	dspop_profileover* op = (dspop_profileover*) _op;
	if (op->filename    != NULL) free (op->filename);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

void op_profileover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_profileover* op = (dspop_profileover*) _op;
	char* name = _op->name;
	const int offLo    = (int) -op->where.upstream;
	const u32 noffsets = (u32) (op->where.upstream + op->where.downstream + 1);
	const u32 bin      = (u32) op->where.bin, ncols = noffsets / bin;

	to_whole ();                                               /* an anchor's window lies in one whole chromosome */
	sigpart* parts;
	int nsrc = signal_parts (&parts);
	anchors* anc = (anchors*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(anchors)), name);

	/* the file: every interval's anchor, to its chromosome */
	u64 numRead, numUsed, numSkipped;
	read_anchor_file (name, op->filename, &op->where, parts, nsrc, anc, &numRead, &numUsed, &numSkipped, NULL, NULL);

	/* both passes */
	gdsp_profile_source* src = (gdsp_profile_source*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(gdsp_profile_source)), name);
	uint64_t* count = (uint64_t*) must_alloc (calloc (ncols, sizeof(uint64_t)), name);
	double*   figs  = (double*)   must_alloc (calloc (4 * (size_t) ncols, sizeof(double)), name);
	double *sum = figs, *mean = figs + ncols, *variance = figs + 2 * (size_t) ncols, *stddev = figs + 3 * (size_t) ncols;
	sync_all_devices ();
	for (int i=0 ; i<nsrc ; i++)
		{
		select_device_of (parts[i].s);
		src[i].d_v = parts[i].v;  src[i].n = parts[i].n;
		src[i].device = physical_device_of (parts[i].s);  src[i].stream = op_stream ();
		src[i].h_pos = anc[i].pos;  src[i].h_minus = anc[i].minus;  src[i].nanchors = anc[i].count;
		}
	if (nsrc > 0) select_device_of (parts[0].s);
	void* reduceCtx = NULL;
	gdsp_reduce_fn reduce = reduce_over_devices (&reduceCtx);      /* (also hands the communicator to the library) */
	check_gdsp (gdsp_genome_profile (src, nsrc, offLo, noffsets, bin, op->sample.minAllowed, op->sample.maxAllowed, reduce, reduceCtx,
	                                 count, sum, mean, variance, stddev), name);
	op->pairs = numUsed * noffsets;
	free (src);
	for (int i=0 ; i<nsrc ; i++) { free (anc[i].pos);  free (anc[i].minus); }
	free (anc);

	/* the table */
	FILE* out = open_table (name, op->outFilename);
	fprintf (out, "# anchors read %llu\n# anchors used %llu\n# anchors skipped %llu\n",
	         (unsigned long long) numRead, (unsigned long long) numUsed, (unsigned long long) numSkipped);
	fprintf (out, "# offsets %d..%d\n# bin %u\n", offLo, offLo + (int) noffsets - 1, bin);
	fprintf (out, "#lo\thi\tcount\tsum\tmean\tstddev\tstderr\n");
	int    haveBest = false, bestOffset = 0;
	double bestMean = 0;
	char   text[2400];
	for (u32 j=0 ; j<ncols ; j++)
		{
		const int lo = offLo + (int) (j * bin);
		char* p = text + snprintf (text, 40, "%d\t%d\t", lo, lo + (int) bin);
		p = put_unsigned (p, count[j]);
		*(p++) = '\t';  p = put_value (p, sum[j], op->sample.precision);
		if (count[j] == 0) { memcpy (p, "\tNA\tNA\tNA", 9);  p += 9; }
		else
			{
			*(p++) = '\t';  p = put_value (p, mean[j],   op->sample.precision);
			*(p++) = '\t';  p = put_value (p, stddev[j], op->sample.precision);
			*(p++) = '\t';  p = put_value (p, stddev[j] / sqrt ((double) count[j]), op->sample.precision);
			}
		*(p++) = '\n';
		fwrite (text, 1, (size_t) (p - text), out);
		if (isnan (mean[j])) continue;
		if (!haveBest || (mean[j] > bestMean)) { bestMean = mean[j];  bestOffset = lo;  haveBest = true; }
		}
	close_table (out);

	set_named_global ("anchors", (valtype) numUsed);
	if (haveBest)
		{
		const struct { char* name;  double x; } best[2] = { { "bestoffset", (double) bestOffset }, { "bestmean", bestMean } };
		char a[400];
		for (int k=0 ; k<2 ; k++)
			{
			set_named_global (best[k].name, best[k].x);
			if (op->sample.quiet) continue;
			format_value (a, sizeof(a), best[k].x, op->sample.precision);
			if (op->reportForBash) fprintf (stdout, "%s=%s # bash command\n", best[k].name, a);
			else                   fprintf (stderr, "%s is %s\n", best[k].name, a);
			}
		}
	else
		fprintf (stderr, "[%s] nothing can be computed;  no anchor finds a value at any of the offsets\n", name);
	free (count);  free (figs);
	}

/* the driver: the signal is only read, twice, 8 B per anchor and offset */
static void profileover_work (dspop* op, u64* bases, double* bytesPerBase)
	{ *bases = ((dspop_profileover*) op)->pairs;  ((dspop_profileover*) op)->pairs = 0;  *bytesPerBase = 16; }

static const dspinfo profileoverRows[] =
	{ dspinforecord("profileover", op_profileover), dspinfoalias ("profile_over"), dspinfoalias ("aggregate"),
	  dspinfoalias ("metaprofile"), dspinfoalias ("metagene") };
static const optraits profileoverTraits[] = { { op_profileover_apply, true, false, NULL, NULL, profileover_work } };
const opgroup opgroup_profileover = OPGROUP (profileoverRows, profileoverTraits, gdsp_genome_profile_use_comm);
