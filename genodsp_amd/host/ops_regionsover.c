/* ops_regionsover.c -- regionsover (device shim).  Not an operator of the reference: every region a file names -- a gene,
 * a peak, a domain -- stretched or squeezed onto the same number of columns, with unscaled flanks before and behind it:
 * the regions x columns table of deepTools' computeMatrix scale-regions, which every metagene plot and every gene-body
 * heatmap starts from.  It is the other half of matrixover, which looks around a point: one table line per used region,
 * in the file's order, and on it one figure (mean, sum, count, min or max) per column, in the region's own direction.
 * The signal is not modified.
 *
 * The file's lines are read as profileover and matrixover read them (read_anchor_line, ops_common.c), and the options
 * that are theirs too are taken by anchor_opts_take; what a region is and which are used is decided here -- the reader
 * stays here because it counts a line on a chromosome the genome lacks as read and skipped, which read_anchor_file does
 * not count at all.  The whole table is held on the host, 8 bytes a cell, so a call of more than 2^30 cells is refused
 * before any device work.  --as=, that refusal, the storage of the rows, the lines of the table and the report at the end
 * are the row-table half shared with matrixover (host_services.h, ops_common.c).
 *
 * The figures are gdsp_genome_regions' (include/genodsp_hip.h): each value is statsover's figure of the cell's interval,
 * exact and rounded once, a function of the cell's sample alone -- so what is printed does not depend on the number of
 * devices, on the cut of the genome or on chromosome order, and permuting the file's lines permutes the rows.
 *
 * The driver finds this operator through opgroup_regionsover, at the end of this file (host_services.h); every call into
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

dspprototypes(op_regionsover)

typedef struct dspop_regionsover
	{
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                         /* (its limits, precision and quiet; no window) */
	anchor_opts where;                          /* the flanks, their bin, the strand column and the origin (host_services.h) */
	long long   body, minLength;
	int         what;                           /* GDSP_MATRIX_* */
	u64         bases, cells;                   /* bases looked at and cells written by the last call (--report=gpu) */
	} dspop_regionsover;

OP_SHORT (op_regionsover, "print each region a file names scaled to the same columns, one row per region (not in genodsp)")

void op_regionsover_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sEvery region a file names, scaled to the same number of columns (the regions x columns matrix\n", indent);
	fprintf (f, "%sbehind a metagene plot or a gene-body heatmap): every interval of the file gives one line of\n", indent);
	fprintf (f, "%sthe table, in the file's order; on it one figure for every column of the upstream flank, of\n", indent);
	fprintf (f, "%sthe region's own bases divided into --body columns, and of the downstream flank -- in the\n", indent);
	fprintf (f, "%sregion's own direction when a strand column is named. Body column k of a region of L bases\n", indent);
	fprintf (f, "%sholds bases floor(k L / body) up to floor((k+1) L / body) from its start. Every sum is exact\n", indent);
	fprintf (f, "%sand rounded once. A line is: chrom start end strand length, then the columns (NA where\n", indent);
	fprintf (f, "%snothing was found). A region that leaves its chromosome is skipped; a flank that does keeps\n", indent);
	fprintf (f, "%sthe bases inside. The variables regions and cells are set. The signal is not modified. Not\n", indent);
	fprintf (f, "%sin genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> --body=<columns> [options]\n", indent, name);
	fprintf (f, "%s  --body=<columns>         columns every region is scaled to, 1 .. %d\n", indent, GDSP_REGIONS_MAX_COLUMNS);
	fprintf (f, "%s  --flank=<bases>          unscaled bases before and behind the region (default: 0)\n", indent);
	fprintf (f, "%s  --upstream=<bases> --downstream=<bases>  the same, each on its own; at most %d\n", indent, GDSP_REGIONS_MAX_COLUMNS);
	fprintf (f, "%s  --bin=<bases>            flank bases per column; must divide both flanks (default: 1)\n", indent);
	fprintf (f, "%s  --strand=<col>           column <col> of the file holds the strand; a field that begins\n", indent);
	fprintf (f, "%s                           with - is the minus strand (default: every region is plus)\n", indent);
	fprintf (f, "%s  --minlength=<bases>      skip regions shorter than this (default: 1)\n", indent);
	fprintf (f, "%s  --as=mean|sum|count|min|max  the figure of a cell (default: mean)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout)\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        intervals are origin-one, closed / origin-zero, half-open\n", indent);
	fprintf (f, "%s  --quiet                  do not report regions and cells on stderr\n", indent);
	}

dspop* op_regionsover_parse (char* name, int argc, char** argv)
	{
	dspop_regionsover* op = (dspop_regionsover*) new_op (name, sizeof(dspop_regionsover), true);
	sample_opts_init (&op->sample);
	anchor_opts_init (&op->where);
	op->what = GDSP_MATRIX_MEAN;
	op->body = 0;  op->minLength = 1;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (strcmp_prefix (arg, "--body=") == 0)
			{
			op->body = string_to_unitized_int (argVal, /*thousands*/ true);
			if ((op->body < 1) || (op->body > GDSP_REGIONS_MAX_COLUMNS))
				chastise ("[%s] the body takes 1 .. %d columns (\"%s\")\n", name, GDSP_REGIONS_MAX_COLUMNS, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--minlength=") == 0)
			{
			op->minLength = string_to_unitized_int (argVal, /*thousands*/ true);
			if (op->minLength < 1) chastise ("[%s] the least length must be at least one base (\"%s\")\n", name, arg);
			continue;
			}
		if (strcmp_prefix (arg, "--anchor=") == 0)
			chastise ("[%s] a region is looked at from its start to its end: no anchor (\"%s\")\n", name, arg);
		if (anchor_opts_take (&op->where, name, arg)) continue;        /* (flanks, --bin=, --strand=, --origin=; refuses a window) */
		if (figure_opt_take (name, arg, &op->what)) continue;
		if (strcmp_prefix (arg, "--output=") == 0)
			{ if (op->outFilename != NULL) free (op->outFilename);  op->outFilename = copy_string (argVal);  continue; }
		if (sample_opts_take (&op->sample, name, arg, SAMPLE_OPT_PRECISION | SAMPLE_OPT_QUIET)) continue;
		if (strcmp_prefix (arg, "--debug") == 0) continue;
		if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		if (op->filename == NULL) { op->filename = copy_string (arg);  continue; }
		chastise ("[%s] Can't understand \"%s\"\n", name, arg);
		}
	if (op->filename == NULL) chastise ("[%s] no filename was provided\n", name);
	if (op->body == 0) chastise ("[%s] no body was provided (--body=<columns>)\n", name);
	anchor_opts* w = &op->where;
	if (w->haveFlank && (w->haveUp || w->haveDown))
		chastise ("[%s] Can't use --flank with --upstream or --downstream\n", name);
	if (w->haveFlank) w->upstream = w->downstream = w->flank;       /* (neither given: no flank on that side) */
	if ((w->upstream > GDSP_REGIONS_MAX_COLUMNS) || (w->downstream > GDSP_REGIONS_MAX_COLUMNS))
		chastise ("[%s] a flank can have at most %d bases (%lld upstream, %lld downstream)\n", name, GDSP_REGIONS_MAX_COLUMNS, w->upstream, w->downstream);
	if ((w->upstream % w->bin != 0) || (w->downstream % w->bin != 0))
		chastise ("[%s] the bin must divide both flanks (%lld does not divide %lld and %lld)\n", name, w->bin, w->upstream, w->downstream);
	const long long ncols = w->upstream / w->bin + op->body + w->downstream / w->bin;
	if (ncols > GDSP_REGIONS_MAX_COLUMNS)
		chastise ("[%s] at most %d columns can be computed at once (%lld + %lld + %lld)\n", name, GDSP_REGIONS_MAX_COLUMNS,
		          w->upstream / w->bin, op->body, w->downstream / w->bin);
	if (op->sample.minAllowed > op->sample.maxAllowed) chastise ("[%s] --min can't be above --max\n", name);
	return (dspop*) op;
	}

void op_regionsover_free (dspop* _op)
	{
	dspop_regionsover* op = (dspop_regionsover*) _op;
	if (op->filename    != NULL) free (op->filename);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

/* the regions of one chromosome as the library takes them */
typedef struct regions { u32 *start, *end, *minus;  u32 count, cap; } regions;

void op_regionsover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_regionsover* op = (dspop_regionsover*) _op;
	char* name = _op->name;
	const u32 B = (u32) op->body, U = (u32) op->where.upstream, D = (u32) op->where.downstream, bin = (u32) op->where.bin;
	const u32 nUp = U / bin, nDown = D / bin, ncols = nUp + B + nDown;
	const long long org = op->where.originOne? 1 : 0;

	to_whole ();                                               /* a region and its flanks lie in one whole chromosome */
	sigpart* parts;
	int nsrc = signal_parts (&parts);
	regions* reg = (regions*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(regions)), name);
	rowlist  list = { NULL, 0, 0, name };                     /* the used regions in the file's order */
	u64 numRead = 0, numSkipped = 0, basesSeen = 0;

	/* the file: a region is used when its chromosome is in the genome, it lies inside it and it is long enough */
	FILE* f = fopen (op->filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", name, op->filename);  exit (EXIT_FAILURE); }
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;
	char  line[1001], prevChrom[1001];
	char* chrom;
	u32   start, end;
	int   minus, at = -1;
	u64   lineNumber = 0;
	spec* s = NULL;
	prevChrom[0] = 0;
	while (read_anchor_line (name, op->filename, f, line, sizeof(line), &lineNumber, op->where.strandColumn, &chrom, &start, &end, &minus))
		{
		if (strcmp (chrom, prevChrom) != 0)
			{
			s = find_chromosome_spec (chrom);  safe_strncpy (prevChrom, chrom, sizeof(prevChrom)-1);
			at = -1;
			for (int i=0 ; (s!=NULL) && (i<nsrc) ; i++) { if (parts[i].s == s) { at = i;  break; } }
			if (at < 0) s = NULL;
			}
		numRead++;
		if (s == NULL) { numSkipped++;  continue; }
		if (!s->flag) { if (trackOperations) fprintf (stderr, "%s(%s)\n", name, chrom);  s->flag = true; }
		const long long is = (long long) start - org - (long long) s->start, ie = (long long) end - (long long) s->start;
		if ((is < 0) || (is >= ie) || (ie > (long long) parts[at].n) || (ie - is < op->minLength)) { numSkipped++;  continue; }
		regions* a = &reg[at];
		if (a->count == a->cap)
			{
			if (a->cap >= (1u << 31)) { fprintf (stderr, "[%s] too many regions on %s\n", name, chrom);  exit (EXIT_FAILURE); }
			a->cap   = (a->cap == 0)? 1024 : 2*a->cap;
			a->start = (u32*) must_alloc (realloc (a->start, a->cap * sizeof(u32)), name);
			a->end   = (u32*) must_alloc (realloc (a->end,   a->cap * sizeof(u32)), name);
			a->minus = (u32*) must_alloc (realloc (a->minus, a->cap * sizeof(u32)), name);
			}
		rowlist_add (&list, at, a->count, start, end, (u32) (ie - is), minus);
		a->start[a->count] = (u32) is;  a->end[a->count] = (u32) ie;  a->minus[a->count] = (u32) minus;  a->count++;
		basesSeen += (u64) U + (u64) (ie - is) + (u64) D;
		}
	fclose (f);
	const u64 numUsed = list.count;
	const u64 cells = row_table_cells (name, numUsed, ncols,
	                                   "[%s] %llu regions times %u columns are %llu cells, more than the %llu a call can hold; use a smaller --body or a wider --bin\n");

	gdsp_region_source* src = (gdsp_region_source*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(gdsp_region_source)), name);
	double** table = (double**) must_alloc (calloc (nsrc? nsrc : 1, sizeof(double*)), name);
	sync_all_devices ();
	for (int i=0 ; i<nsrc ; i++)
		{
		table[i] = row_table_part (name, &parts[i], reg[i].count, ncols, &src[i].d_v, &src[i].n, &src[i].device, &src[i].stream);
		src[i].h_start = reg[i].start;  src[i].h_end = reg[i].end;  src[i].h_minus = reg[i].minus;  src[i].nregions = reg[i].count;
		}
	if (nsrc > 0) select_device_of (parts[0].s);
	check_gdsp (gdsp_genome_regions (src, nsrc, B, U, D, bin, op->what, op->sample.minAllowed, op->sample.maxAllowed, table), name);
	op->bases = basesSeen;  op->cells = cells;
	free (src);
	for (int i=0 ; i<nsrc ; i++) { free (reg[i].start);  free (reg[i].end);  free (reg[i].minus); }
	free (reg);

	/* the table */
	FILE* out = open_table (name, op->outFilename);
	fprintf (out, "# regions read %llu\n# regions used %llu\n# regions skipped %llu\n",
	         (unsigned long long) numRead, (unsigned long long) numUsed, (unsigned long long) numSkipped);
	fprintf (out, "# upstream %u\n# body %u\n# downstream %u\n# bin %u\n# as %s\n", U, B, D, bin, figureNames[op->what]);
	fprintf (out, "#chrom\tstart\tend\tstrand\tlength");
	for (u32 j=0 ; j<nUp ; j++)   fprintf (out, "\t%lld", -(long long) U + (long long) j * bin);
	for (u32 j=0 ; j<B ; j++)     fprintf (out, "\tb%u", j);
	for (u32 j=0 ; j<nDown ; j++) fprintf (out, "\t+%u", j * bin);
	fprintf (out, "\n");
	row_table_print (name, out, &list, table, ncols, parts, op->where.strandColumn, /*withLength*/ true, op->sample.precision);
	close_table (out);
	for (int i=0 ; i<nsrc ; i++) free (table[i]);
	free (table);
	free (list.rows);
	row_table_report ("regions", numUsed, cells, op->sample.quiet);
	}

/* the driver: the signal is only read, 8 B per base of a region and its flanks, and 8 B are written per cell */
static void regionsover_work (dspop* _op, u64* bases, double* bytesPerBase)
	{
	dspop_regionsover* op = (dspop_regionsover*) _op;
	*bases = op->bases;
	*bytesPerBase = 8 + ((op->bases != 0)? 8.0 * (double) op->cells / (double) op->bases : 0.0);
	op->bases = op->cells = 0;
	}

static const dspinfo regionsoverRows[] =
	{ dspinforecord("regionsover", op_regionsover), dspinfoalias ("regions_over"), dspinfoalias ("scaleregions"),
	  dspinfoalias ("scale_regions"), dspinfoalias ("genebodies") };
static const optraits regionsoverTraits[] = { { op_regionsover_apply, true, false, NULL, NULL, regionsover_work } };
const opgroup opgroup_regionsover = OPGROUP (regionsoverRows, regionsoverTraits, NULL);
