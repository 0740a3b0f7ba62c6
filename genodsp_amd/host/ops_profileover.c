/* ops_profileover.c -- profileover (device shim).  Not an operator of the reference: what the signal looks like, on
 * average, around the positions a file names -- read depth from 2 kb before to 2 kb behind every transcription start,
 * oriented by strand; the footprint around a million motif sites (the aggregate profile, or metaplot, of deepTools'
 * computeMatrix + plotProfile).  One table line per column of offsets: count, sum, mean, stddev and stderr of the values
 * found that far from the anchors, in each anchor's own direction.  The signal is not modified.
 *
 * The file is read and routed as statsover reads its own (origin, chromosomes the run does not hold are skipped, the trace
 * lines), but by a reader of this file's, which also fetches the strand column; read_interval is left as it is.  Each
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

enum { anchor_start = 0, anchor_end = 1, anchor_center = 2 };

typedef struct dspop_profileover
	{
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                         /* (its limits, precision and quiet; no window) */
	int         originOne, reportForBash;
	int         haveFlank, haveUp, haveDown;
	long long   flank, upstream, downstream;
	int         anchor, strandColumn;           /* strandColumn: zero-based, -1 when every anchor is plus */
	long long   bin;
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

static long long bases_arg (char* name, char* arg, char* argVal, const char* what)
	{
	int n = string_to_unitized_int (argVal, /*thousands*/ true);
	if (n < 0) chastise ("[%s] %s can't be negative (\"%s\")\n", name, what, arg);
	return n;
	}

dspop* op_profileover_parse (char* name, int argc, char** argv)
	{
	dspop_profileover* op = (dspop_profileover*) new_op (name, sizeof(dspop_profileover), true);
	sample_opts_init (&op->sample);
	op->originOne    = (int) get_named_global ("originOne", false);
	op->strandColumn = -1;
	op->anchor       = anchor_start;
	op->bin          = 1;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (strcmp_prefix (arg, "--flank=") == 0)      { op->flank      = bases_arg (name, arg, argVal, "the flank");           op->haveFlank = true;  continue; }
		if (strcmp_prefix (arg, "--upstream=") == 0)   { op->upstream   = bases_arg (name, arg, argVal, "the upstream reach");   op->haveUp    = true;  continue; }
		if (strcmp_prefix (arg, "--downstream=") == 0) { op->downstream = bases_arg (name, arg, argVal, "the downstream reach"); op->haveDown  = true;  continue; }
		if (strcmp_prefix (arg, "--bin=") == 0)
			{
			int b = string_to_unitized_int (argVal, /*thousands*/ true);
			if (b < 1) chastise ("[%s] the bin must be at least one base (\"%s\")\n", name, arg);
			op->bin = b;
			continue;
			}
		if (strcmp_prefix (arg, "--anchor=") == 0)
			{
			if      (strcmp (argVal, "start")  == 0) op->anchor = anchor_start;
			else if (strcmp (argVal, "end")    == 0) op->anchor = anchor_end;
			else if ((strcmp (argVal, "center") == 0) || (strcmp (argVal, "centre") == 0)) op->anchor = anchor_center;
			else chastise ("[%s] the anchor is the interval's start, end or center (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--strand=") == 0)
			{
			int col = string_to_int (argVal) - 1;
			if (col == -1) chastise ("[%s] strand column can't be 0 (\"%s\")\n", name, arg);
			if (col < 0)   chastise ("[%s] strand column can't be negative (\"%s\")\n", name, arg);
			if (col < 3)   chastise ("[%s] strand column can't be 1, 2 or 3 (\"%s\")\n", name, arg);
			op->strandColumn = col;
			continue;
			}
		if (is_opt3 (arg, "window", "W"))
			chastise ("[%s] every base the anchors reach is looked at: no window (\"%s\")\n", name, arg);
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if ((strcmp (arg, "--report:bash") == 0) || (strcmp (arg, "--bash") == 0)) { op->reportForBash = true;  continue; }
		if (sample_opts_take (&op->sample, name, arg, SAMPLE_OPT_PRECISION | SAMPLE_OPT_QUIET)) continue;
		if (origin_opt_take (arg, &op->originOne)) continue;
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (op->filename == NULL) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->filename == NULL) chastise ("[%s] no filename was provided\n", name);
	if (op->haveFlank && (op->haveUp || op->haveDown))
		chastise ("[%s] Can't use --flank with --upstream or --downstream\n", name);
	if (!op->haveFlank && !(op->haveUp && op->haveDown))
		chastise ("[%s] no offsets were provided (--flank=<bases>, or --upstream=<bases> and --downstream=<bases>)\n", name);
	if (op->haveFlank) op->upstream = op->downstream = op->flank;
	const long long noffsets = op->upstream + op->downstream + 1;
	if (noffsets > GDSP_PROFILE_MAX_OFFSETS)
		chastise ("[%s] at most %d offsets can be computed at once (%lld..%lld)\n", name, GDSP_PROFILE_MAX_OFFSETS, -op->upstream, op->downstream);
	if (noffsets % op->bin != 0)
		chastise ("[%s] the bin must divide the number of offsets (%lld does not divide %lld)\n", name, op->bin, noffsets);
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

/* ------------------------------------------------------------------------------------------ the file ---- */
/* a line of the file as read_interval's serial loop (ingest.c) takes it -- track lines, blank lines and comments are
 * passed over; chromosome, start and end are the first three fields -- and with it the strand: minus when field
 * strandCol (zero-based; -1: none) begins with '-'.  false at the end of the file */
static int read_anchor_line (char* name, char* filename, FILE* f, char* line, int lineLen, u64* lineNumber, int strandCol,
                             char** _chrom, u32* _start, u32* _end, int* _minus)
	{
	char *scan, *mark, *field;
	for (;;)
		{
		if (fgets (line, lineLen, f) == NULL) return false;
		(*lineNumber)++;
		size_t len = strlen (line);
		if ((len != 0) && (line[len-1] != '\n') && !feof (f))
			{ fprintf (stderr, "[%s] in \"%s\", line %llu is longer than internal buffer\n", name, filename, (unsigned long long) *lineNumber);  exit (EXIT_FAILURE); }
		if (strcmp_prefix (line, "track ") == 0) continue;
		scan = skip_whitespace (line);
		if ((*scan == 0) || (*scan == '#')) continue;
		break;
		}
	const char* missing = NULL;
	char* chrom = scan = line;
	if (*scan == ' ') missing = "chromosome";
	mark = skip_darkspace (scan);  scan = skip_whitespace (mark);  if (*mark != 0) *mark = 0;
	if ((missing == NULL) && (*scan == 0)) missing = "interval start";
	field = scan;
	mark = skip_darkspace (scan);  scan = skip_whitespace (mark);  if (*mark != 0) *mark = 0;
	u32 start = (missing == NULL)? (u32) string_to_u32 (field) : 0;
	if ((missing == NULL) && (*scan == 0)) missing = "interval end";
	field = scan;
	mark = skip_darkspace (scan);  scan = skip_whitespace (mark);  if (*mark != 0) *mark = 0;
	u32 end = (missing == NULL)? (u32) string_to_u32 (field) : 0;
	int minus = false;
	for (int col=3 ; (missing == NULL) && (col<=strandCol) ; col++)
		{
		if (*scan == 0) { missing = "strand";  break; }
		field = scan;
		mark = skip_darkspace (scan);  scan = skip_whitespace (mark);
		if (col == strandCol) minus = (field[0] == '-');
		}
	if (missing != NULL)
		{
		fprintf (stderr, "[%s] in \"%s\", line %llu contains no %s\n", name, filename, (unsigned long long) *lineNumber, missing);
		exit (EXIT_FAILURE);
		}
	*_chrom = chrom;  *_start = start;  *_end = end;  *_minus = minus;
	return true;
	}

/* where the anchor of the zero-based half-open interval [s, e), s < e, lies */
static long long anchor_of (long long s, long long e, int minus, int anchor)
	{
	const long long half = (e - s - 1) / 2;
	switch (anchor)
		{
		case anchor_end:    return minus? s : e - 1;
		case anchor_center: return minus? e - 1 - half : s + half;
		default:            return minus? e - 1 : s;
		}
	}

/* a chromosome's anchors, as the library takes them */
typedef struct anchors { u32 *pos, *minus;  u32 count, cap; } anchors;

void op_profileover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_profileover* op = (dspop_profileover*) _op;
	char* name = _op->name;
	const int       offLo    = (int) -op->upstream;
	const u32       noffsets = (u32) (op->upstream + op->downstream + 1);
	const u32       bin      = (u32) op->bin, ncols = noffsets / bin;
	const long long o        = op->originOne? 1 : 0;

	to_whole ();                                               /* an anchor's window lies in one whole chromosome */
	sigpart* parts;
	int nsrc = signal_parts (&parts);
	anchors* anc = (anchors*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(anchors)), name);

	/* the file: every interval's anchor, to its chromosome */
	FILE* f = fopen (op->filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", name, op->filename);  exit (EXIT_FAILURE); }
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;
	char  line[1001], prevChrom[1001];
	char* chrom;
	u32   start, end;
	int   minus, at = -1;
	u64   lineNumber = 0, numRead = 0, numUsed = 0, numSkipped = 0;
	spec* s = NULL;
	prevChrom[0] = 0;
	while (read_anchor_line (name, op->filename, f, line, sizeof(line), &lineNumber, op->strandColumn, &chrom, &start, &end, &minus))
		{
		if (strcmp (chrom, prevChrom) != 0)
			{
			s = find_chromosome_spec (chrom);  safe_strncpy (prevChrom, chrom, sizeof(prevChrom)-1);
			at = -1;
			for (int i=0 ; (s!=NULL) && (i<nsrc) ; i++) { if (parts[i].s == s) { at = i;  break; } }
			if (at < 0) s = NULL;
			}
		if (s == NULL) continue;
		if (!s->flag) { if (trackOperations) fprintf (stderr, "%s(%s)\n", name, chrom);  s->flag = true; }
		numRead++;
		const long long is = (long long) start - o, ie = (long long) end;
		long long p = -1;
		if (is < ie) p = anchor_of (is, ie, minus, op->anchor) - (long long) s->start;
		if ((is >= ie) || (p < 0) || (p >= (long long) parts[at].n)) { numSkipped++;  continue; }
		anchors* a = &anc[at];
		if (a->count == a->cap)
			{
			if (a->cap >= (1u << 31)) { fprintf (stderr, "[%s] too many anchors on %s\n", name, chrom);  exit (EXIT_FAILURE); }
			a->cap   = (a->cap == 0)? 1024 : 2*a->cap;
			a->pos   = (u32*) must_alloc (realloc (a->pos,   a->cap * sizeof(u32)), name);
			a->minus = (u32*) must_alloc (realloc (a->minus, a->cap * sizeof(u32)), name);
			}
		a->pos[a->count] = (u32) p;  a->minus[a->count] = (u32) minus;  a->count++;
		numUsed++;
		}
	fclose (f);

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
