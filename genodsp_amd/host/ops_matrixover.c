/* ops_matrixover.c -- matrixover (device shim).  Not an operator of the reference: the signal around each of the
 * positions a file names, anchor by anchor -- the anchors x bins table of deepTools' computeMatrix, which every heatmap
 * and every clustering of promoters starts from.  It is profileover's picture before the anchors are added up: one table
 * line per used anchor, in the file's order, and on it one figure (mean, sum, count, min or max) per column of offsets,
 * in the anchor's own direction.  The signal is not modified.
 *
 * Options, refusals and the file's reader are profileover's (anchor_opts and read_anchor_file, ops_common.c).  The whole
 * matrix is held on the host, 8 bytes a cell, so a call of more than 2^30 cells is refused before any device work.  --as=,
 * that refusal, the storage of the rows, the lines of the table and the report at the end are the row-table half shared
 * with regionsover (host_services.h, ops_common.c).
 *
 * The figures are gdsp_genome_matrix's (include/genodsp_hip.h): each value is statsover's figure of the cell's interval,
 * exact and rounded once, a function of the cell's sample alone -- so what is printed does not depend on the number of
 * devices, on the cut of the genome or on chromosome order, and permuting the file's lines permutes the rows.
 *
 * The driver finds this operator through opgroup_matrixover, at the end of this file (host_services.h); every call into
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

dspprototypes(op_matrixover)

typedef struct dspop_matrixover
	{
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                         /* (its limits, precision and quiet; no window) */
	anchor_opts where;                          /* the anchors and the offsets around them (host_services.h) */
	int         what;                           /* GDSP_MATRIX_* */
	u64         pairs;                          /* anchors times offsets of the last call (--report=gpu) */
	} dspop_matrixover;

OP_SHORT (op_matrixover, "print the exact signal around each anchor a file names, one row per anchor (not in genodsp)")

void op_matrixover_usage (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sThe signal around the positions a file names, anchor by anchor (the anchors x bins matrix\n", indent);
	fprintf (f, "%sbehind a heatmap): every interval of the file gives one anchor and one line of the table, in\n", indent);
	fprintf (f, "%sthe file's order; on it, for every column of offsets, one figure of the values found that far\n", indent);
	fprintf (f, "%sfrom the anchor -- downstream is the anchor's own direction when a strand column is named.\n", indent);
	fprintf (f, "%sEvery sum is exact and rounded once. A line is: chrom start end strand, then the columns (NA\n", indent);
	fprintf (f, "%swhere nothing was found). A window that leaves its chromosome keeps the offsets that stay\n", indent);
	fprintf (f, "%sinside. The variables anchors and cells are set. The signal is not modified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> --flank=<bases> | --upstream=<bases> --downstream=<bases> [options]\n", indent, name);
	fprintf (f, "%s  --flank=<bases>          offsets -<bases> .. <bases>\n", indent);
	fprintf (f, "%s  --upstream=<bases> --downstream=<bases>  offsets -<upstream> .. <downstream>, at most %d\n", indent, GDSP_PROFILE_MAX_OFFSETS);
	fprintf (f, "%s  --anchor=start|end|center  where in its interval the anchor lies, in the interval's own\n", indent);
	fprintf (f, "%s                           direction (default: start)\n", indent);
	fprintf (f, "%s  --strand=<col>           column <col> of the file holds the strand; a field that begins\n", indent);
	fprintf (f, "%s                           with - is the minus strand (default: every anchor is plus)\n", indent);
	fprintf (f, "%s  --bin=<bases>            offsets per column; must divide their number (default: 1)\n", indent);
	fprintf (f, "%s  --as=mean|sum|count|min|max  the figure of a cell (default: mean)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout)\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        intervals are origin-one, closed / origin-zero, half-open\n", indent);
	fprintf (f, "%s  --quiet                  do not report anchors and cells on stderr\n", indent);
	}

dspop* op_matrixover_parse (char* name, int argc, char** argv)
	{
	dspop_matrixover* op = (dspop_matrixover*) new_op (name, sizeof(dspop_matrixover), true);
	sample_opts_init (&op->sample);
	anchor_opts_init (&op->where);
	op->what = GDSP_MATRIX_MEAN;
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if (anchor_opts_take (&op->where, name, arg)) continue;
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
	anchor_opts_check (&op->where, name);
	if (op->sample.minAllowed > op->sample.maxAllowed) chastise ("[%s] --min can't be above --max\n", name);
	return (dspop*) op;
	}

void op_matrixover_free (dspop* _op)
	{
	dspop_matrixover* op = (dspop_matrixover*) _op;
	if (op->filename    != NULL) free (op->filename);
	if (op->outFilename != NULL) free (op->outFilename);
	free (op);
	}

/* the used anchors in the file's order: whose row each is, and its interval as the file has it */
static void remember_row (void* ctx, int part, u32 index, u32 start, u32 end, int minus)
	{ rowlist_add ((rowlist*) ctx, part, index, start, end, /*length*/ 0, minus); }

void op_matrixover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_matrixover* op = (dspop_matrixover*) _op;
	char* name = _op->name;
	const int offLo    = (int) -op->where.upstream;
	const u32 noffsets = (u32) (op->where.upstream + op->where.downstream + 1);
	const u32 bin      = (u32) op->where.bin, ncols = noffsets / bin;

	to_whole ();                                               /* an anchor's window lies in one whole chromosome */
	sigpart* parts;
	int nsrc = signal_parts (&parts);
	anchors* anc = (anchors*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(anchors)), name);
	rowlist list = { NULL, 0, 0, name };
	u64 numRead, numUsed, numSkipped;
	read_anchor_file (name, op->filename, &op->where, parts, nsrc, anc, &numRead, &numUsed, &numSkipped, remember_row, &list);
	const u64 cells = row_table_cells (name, numUsed, ncols,
	                                   "[%s] %llu anchors times %u columns are %llu cells, more than the %llu a call can hold; use a wider --bin\n");

	gdsp_profile_source* src = (gdsp_profile_source*) must_alloc (calloc (nsrc? nsrc : 1, sizeof(gdsp_profile_source)), name);
	double** rows = (double**) must_alloc (calloc (nsrc? nsrc : 1, sizeof(double*)), name);
	sync_all_devices ();
	for (int i=0 ; i<nsrc ; i++)
		{
		rows[i] = row_table_part (name, &parts[i], anc[i].count, ncols, &src[i].d_v, &src[i].n, &src[i].device, &src[i].stream);
		src[i].h_pos = anc[i].pos;  src[i].h_minus = anc[i].minus;  src[i].nanchors = anc[i].count;
		}
	if (nsrc > 0) select_device_of (parts[0].s);
	check_gdsp (gdsp_genome_matrix (src, nsrc, offLo, noffsets, bin, op->what, op->sample.minAllowed, op->sample.maxAllowed, rows), name);
	op->pairs = numUsed * noffsets;
	free (src);
	for (int i=0 ; i<nsrc ; i++) { free (anc[i].pos);  free (anc[i].minus); }
	free (anc);

	/* the table */
	FILE* out = open_table (name, op->outFilename);
	fprintf (out, "# anchors read %llu\n# anchors used %llu\n# anchors skipped %llu\n",
	         (unsigned long long) numRead, (unsigned long long) numUsed, (unsigned long long) numSkipped);
	fprintf (out, "# offsets %d..%d\n# bin %u\n# as %s\n", offLo, offLo + (int) noffsets - 1, bin, figureNames[op->what]);
	fprintf (out, "#chrom\tstart\tend\tstrand");
	for (u32 j=0 ; j<ncols ; j++) fprintf (out, "\t%d", offLo + (int) (j * bin));
	fprintf (out, "\n");
	row_table_print (name, out, &list, rows, ncols, parts, op->where.strandColumn, /*withLength*/ false, op->sample.precision);
	close_table (out);
	for (int i=0 ; i<nsrc ; i++) free (rows[i]);
	free (rows);
	free (list.rows);
	row_table_report ("anchors", numUsed, cells, op->sample.quiet);
	}

/* the driver: the signal is only read, 8 B per anchor and offset, and 8 B are written per cell */
static void matrixover_work (dspop* _op, u64* bases, double* bytesPerBase)
	{
	dspop_matrixover* op = (dspop_matrixover*) _op;
	*bases = op->pairs;  op->pairs = 0;
	*bytesPerBase = 8 + 8.0 / (double) op->where.bin;
	}

static const dspinfo matrixoverRows[] =
	{ dspinforecord("matrixover", op_matrixover), dspinfoalias ("matrix_over"), dspinfoalias ("computematrix"),
	  dspinfoalias ("signalmatrix") };
static const optraits matrixoverTraits[] = { { op_matrixover_apply, true, false, NULL, NULL, matrixover_work } };
const opgroup opgroup_matrixover = OPGROUP (matrixoverRows, matrixoverTraits, NULL);
